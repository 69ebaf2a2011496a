// gps_track -- offline tracking front end: search the first run of a 1-bit real-IF capture, start a tracking channel for every
// hit, track to the end of the file (or SECONDS), and decode NAV bits and subframes (include/gpsacq.h, gpsacq_track*).
//
//     gps_track FILE FC FS [SECONDS]
//
// The search is SearchTask()'s first run (c/search_offline.cpp:237-262: block b of 5120 bytes against PRN b % 32, hits at
// SNR > 25); the reference's live receiver has no stdout surface for tracking, so the output format is this program's own:
//     chan K PRN P status ok|lost epochs E dop_hz D code_hz C bits B
//     subframe PRN P id I tow T
//     parity PRN P failures F
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gpsacq.h"

int main(int argc, char** argv) {
    if (argc < 4 || argc > 5) {
        std::fprintf(stderr, "usage: %s FILE FC FS [SECONDS]\n", argv[0]);
        return 64;
    }
    gpsacq_params prm{};
    prm.fc = std::atof(argv[2]);
    prm.fs = std::atof(argv[3]);
    prm.max_fo = 5000.0;
    const double secs = argc > 4 ? std::atof(argv[4]) : 0.0;
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 66;
    }
    std::fseek(fp, 0, SEEK_END);
    size_t n_bytes = (size_t)std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    if (secs > 0 && (size_t)(secs * prm.fs / 8) < n_bytes) n_bytes = (size_t)(secs * prm.fs / 8);
    std::vector<uint8_t> bits(n_bytes);
    n_bytes = std::fread(bits.data(), 1, n_bytes, fp);
    std::fclose(fp);
    const size_t n_blocks = n_bytes / GPSACQ_BLOCK_BYTES < GPSACQ_NUM_SATS ? n_bytes / GPSACQ_BLOCK_BYTES : GPSACQ_NUM_SATS;
    if (n_blocks == 0) {
        std::fprintf(stderr, "capture shorter than one block\n");
        return 65;
    }
    gpsacq_engine* e = nullptr;
    int rc = gpsacq_create(&prm, &e);
    if (rc) {
        std::fprintf(stderr, "gpsacq_create: %d: %s\n", rc, gpsacq_last_error());
        return rc;
    }
    std::vector<gpsacq_peak> peaks(n_blocks);
    rc = gpsacq_search(e, bits.data(), n_blocks, GPSACQ_BLOCK_BYTES, nullptr, n_blocks, nullptr, peaks.data());
    std::vector<gpsacq_track_chan> chans;
    for (size_t b = 0; rc == 0 && b < n_blocks; ++b) {
        if (!(peaks[b].snr > 25.0f)) continue;
        gpsacq_track_chan ch;
        rc = gpsacq_track_start(e, (int)(b % 32) + 1, &peaks[b], (uint64_t)b * GPSACQ_BLOCK_BYTES * 8, nullptr, &ch);
        chans.push_back(ch);
    }
    gpsacq_info info;
    gpsacq_get_info(e, &info);
    const int max_epochs = (int)(n_bytes * 8 / (size_t)info.num_lags) + 2;
    std::vector<int32_t> prompt(chans.size() * (size_t)max_epochs * 2), n_ep(chans.size());
    if (rc == 0 && !chans.empty())
        rc = gpsacq_track(e, bits.data(), n_bytes, 0, chans.data(), (int)chans.size(), nullptr, prompt.data(), nullptr, max_epochs, n_ep.data());
    if (rc) {
        std::fprintf(stderr, "gps_track: %d: %s\n", rc, gpsacq_last_error());
        gpsacq_destroy(e);
        return rc;
    }
    const double two32 = 4294967296.0;
    for (size_t c = 0; c < chans.size(); ++c) {
        const gpsacq_track_chan& ch = chans[c];
        const int n = n_ep[c];
        std::vector<int32_t> ip(n);
        for (int k = 0; k < n; ++k) ip[k] = prompt[((size_t)c * max_epochs + k) * 2];
        // bit sync after the loops' pull-in (the first second), then the bits and the subframes
        const int skip = n > 1000 ? 1000 : 0;
        const int first_epoch = ch.epoch - n + skip;
        std::vector<uint8_t> nb(n / 20 + 1);
        int e0 = -1, n_bits = 0;
        if (gpsacq_nav_bits(ip.data() + skip, n - skip, first_epoch, 0, nb.data(), (int)nb.size(), &e0, &n_bits) != GPSACQ_OK) n_bits = 0;
        std::printf("chan %zu PRN %d status %s epochs %d dop_hz %.1f code_hz %.3f bits %d\n", c, ch.prn, ch.status ? "lost" : "ok", n,
                    ch.lo_rate / two32 * prm.fs - prm.fc, ch.ca_rate / two32 * prm.fs, n_bits);
        std::vector<gpsacq_subframe> sf(n_bits / 300 + 1);
        int n_sf = 0, n_fail = 0;
        gpsacq_nav_subframes(nb.data(), n_bits, sf.data(), (int)sf.size(), &n_sf, &n_fail);
        for (int k = 0; k < n_sf && k < (int)sf.size(); ++k) std::printf("subframe PRN %d id %d tow %d\n", ch.prn, sf[k].id, sf[k].tow);
        std::printf("parity PRN %d failures %d\n", ch.prn, n_fail);
    }
    gpsacq_destroy(e);
    return 0;
}
