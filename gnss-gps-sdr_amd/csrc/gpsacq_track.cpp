// gpsacq_track.cpp -- the NAV decoder of include/gpsacq.h ("Tracking channels and NAV data"), host only: bit sync and NAV
// bits from the prompt I arm, and the subframe scan of CHANNEL::ParityCheck() (c/channel.cpp:329-353) with the parity
// equations of IS-GPS-200 Table 20-XIV.  The channels themselves (gpsacq_track_start, gpsacq_track) are in gpsacq_engine.cpp
// and track_kernels.hip.
#include <cstring>

#include "../../include/gpsacq.h"
#include "acq_launch.hpp"

namespace {
int fail(int code, const char* msg) { return acq::set_last_error(code, msg); }
}  // namespace

extern "C" int gpsacq_nav_bits(const int32_t* ip, int n_epochs, int first_epoch, int sync_epochs, uint8_t* bits, int max_bits,
                               int* bit_epoch0, int* n_bits) {
    if (!ip || n_epochs < 0 || first_epoch < 0 || !n_bits || (max_bits > 0 && !bits) || !bit_epoch0)
        return fail(GPSACQ_ERR_ARG, "gpsacq_nav_bits: bad argument");
    *n_bits = 0;
    *bit_epoch0 = -1;
    const int ns = (sync_epochs <= 0 || sync_epochs > n_epochs) ? n_epochs : sync_epochs;
    long hist[20] = {0};
    for (int k = 1; k < ns; ++k)
        if ((ip[k - 1] < 0) != (ip[k] < 0)) hist[(first_epoch + k) % 20] += 1;
    int best = 0;
    for (int b = 1; b < 20; ++b)
        if (hist[b] > hist[best]) best = b;
    long second = 0;
    for (int b = 0; b < 20; ++b)
        if (b != best && hist[b] > second) second = hist[b];
    if (hist[best] == 0 || hist[best] < 2 * second) return fail(GPSACQ_ERR_ARG, "gpsacq_nav_bits: no bit sync");
    int k0 = ((best - first_epoch) % 20 + 20) % 20;  // first local epoch in the winning bin
    *bit_epoch0 = first_epoch + k0;
    int nb = 0;
    for (int k = k0; k + 20 <= n_epochs; k += 20, ++nb) {
        int64_t s = 0;
        for (int j = 0; j < 20; ++j) s += ip[k + j];
        if (nb < max_bits) bits[nb] = s < 0 ? 1 : 0;
    }
    *n_bits = nb < max_bits ? nb : max_bits;
    return GPSACQ_OK;
}

namespace {
// IS-GPS-200 Table 20-XIV: D25..D30 from d1..d24 and D29*, D30* (which one of the two each equation takes)
const int kParityStar[6] = {29, 30, 29, 30, 30, 29};
uint32_t mask_of(const int* idx, int n) {  // bit 24 - i holds d_i
    uint32_t m = 0;
    for (int i = 0; i < n; ++i) m |= 1u << (24 - idx[i]);
    return m;
}
struct ParityTable {
    uint32_t m[6];
    ParityTable() {
        static const int e25[] = {1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23};
        static const int e26[] = {2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24};
        static const int e27[] = {1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22};
        static const int e28[] = {2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23};
        static const int e29[] = {1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24};
        static const int e30[] = {3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24};
        m[0] = mask_of(e25, 14);
        m[1] = mask_of(e26, 14);
        m[2] = mask_of(e27, 14);
        m[3] = mask_of(e28, 14);
        m[4] = mask_of(e29, 15);
        m[5] = mask_of(e30, 13);
    }
};
const ParityTable kParity;
}  // namespace

extern "C" int gpsacq_nav_subframes(const uint8_t* bits, int n_bits, gpsacq_subframe* out, int max_out, int* n_out, int* n_parity_fail) {
    if (!bits || n_bits < 0 || !n_out || !n_parity_fail || (max_out > 0 && !out)) return fail(GPSACQ_ERR_ARG, "gpsacq_nav_subframes: bad argument");
    static const uint8_t up[8] = {1, 0, 0, 0, 1, 0, 1, 1};
    *n_out = 0;
    *n_parity_fail = 0;
    int i = 0;
    while (i + 300 <= n_bits) {
        int inv;
        bool m_up = true, m_inv = true;
        for (int k = 0; k < 8; ++k) {
            m_up = m_up && (bits[i + k] & 1) == up[k];
            m_inv = m_inv && (bits[i + k] & 1) == 1 - up[k];
        }
        if (m_up) inv = 0;
        else if (m_inv) inv = 1;
        else {
            i += 1;
            continue;
        }
        uint32_t d29 = (uint32_t)inv, d30 = (uint32_t)inv;
        gpsacq_subframe sf;
        std::memset(&sf, 0, sizeof sf);
        int bad = -1;
        for (int w = 0; w < 10; ++w) {
            const uint8_t* D = bits + i + 30 * w;
            uint32_t d = 0;
            for (int k = 0; k < 24; ++k) d = (d << 1) | ((D[k] & 1u) ^ d30);
            for (int q = 0; q < 6; ++q) {
                const uint32_t star = kParityStar[q] == 29 ? d29 : d30;
                const uint32_t par = star ^ (uint32_t)(__builtin_popcount(d & kParity.m[q]) & 1);
                if (par != (D[24 + q] & 1u)) bad = w;
            }
            if (bad >= 0) break;
            sf.words[w] = d;
            d29 = D[28] & 1u;
            d30 = D[29] & 1u;
        }
        if (bad >= 0) {
            *n_parity_fail += 1;
            i += 30 * (bad + 1);
            continue;
        }
        sf.bit_offset = i;
        sf.inverted = inv;
        sf.tow = (int32_t)(sf.words[1] >> 7);         // word 2 bits 1-17
        sf.id = (int32_t)((sf.words[1] >> 2) & 7u);   // word 2 bits 20-22
        if (*n_out < max_out) out[*n_out] = sf;
        *n_out += 1;
        i += 300;
    }
    return GPSACQ_OK;
}
