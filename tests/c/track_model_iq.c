/* track_model_iq.c -- CPU model of one multi-bit complex tracking channel, written from the text of include/gpsacq.h ("THE CHANNEL
 * MODEL" and "Tracking channels on an 8-bit IQ capture", multi-bit mode), one sample at a time: no dot products, no weight words,
 * no mean correction, no wave reduction.  tests/test_track_iq.py checks it against a numpy restatement of the sums and against
 * tests/c/track_model.c on degenerate captures; tests/test_gpu_track_iq.py checks that gpsacq_track_iq8() agrees with it bit for bit.
 *
 * track_model_iq(iq, n_samples, first_sample, format, dc_i, dc_q, chan, params, chips, prompt, records, max_epochs) runs `chan`
 * over the window iq[2 * n_samples] (samples first_sample ..) and returns the number of epochs it ran; dc_i, dc_q = the integers
 * the model subtracts (nearbyint(mean) when the mean is removed, else 0); chips = the 32 words of the channel's PRN. */
#include <stdint.h>
#include <string.h>

#include "gpsacq.h"

static const uint64_t FULL = 1023ull << 32;

static int chip_at(const uint32_t *chips, uint64_t pos) {
    const uint64_t i = pos >> 32;
    return (chips[i >> 5] >> (i & 31)) & 1;
}

static int out_of(uint64_t v, uint64_t nom, int64_t w) {
    const int64_t d = (int64_t)(v - nom);
    return d > w || d < -w;
}

int track_model_iq(const uint8_t *iq, uint64_t n_samples, uint64_t first_sample, int format, int dc_i, int dc_q, gpsacq_track_chan *ch,
                   const gpsacq_track_params *p, const uint32_t *chips, int32_t *prompt, gpsacq_track_record *records, int max_epochs) {
    const uint64_t end = first_sample + n_samples;
    const int off = format == GPSACQ_IQ_U8 ? 128 : 0;
    uint64_t lo_int = (uint64_t)ch->lo_int, ca_int = (uint64_t)ch->ca_int;
    const uint64_t lo_nom = (uint64_t)ch->lo_nom, ca_nom = (uint64_t)ch->ca_nom;
    int t = 0;
    while (t < max_epochs && ch->status == GPSACQ_TRACK_OK) {
        const uint64_t n = (FULL - ch->ca_pos + ch->ca_rate - 1) / ch->ca_rate;
        if (n < (uint64_t)p->min_epoch || n > (uint64_t)p->max_epoch) {
            ch->status = GPSACQ_TRACK_LOST;
            break;
        }
        if (ch->next_sample + n > end) break;
        int64_t I[3] = {0, 0, 0}, Q[3] = {0, 0, 0};  /* E, P, L */
        for (uint64_t j = 0; j < n; ++j) {
            const uint64_t r = ch->next_sample + j - first_sample;
            const int bi = format == GPSACQ_IQ_U8 ? (int)iq[2 * r] : (int)(int8_t)iq[2 * r];
            const int bq = format == GPSACQ_IQ_U8 ? (int)iq[2 * r + 1] : (int)(int8_t)iq[2 * r + 1];
            const int vi = bi - off - dc_i, vq = bq - off - dc_q;
            const uint32_t ph = ch->lo_phase + (uint32_t)j * ch->lo_rate;
            const int C = 1 - 2 * (int)(((ph >> 31) ^ (ph >> 30)) & 1u);
            const int S = 1 - 2 * (int)(((ph >> 31) & 1u) ^ 1u);
            const uint64_t P = ch->ca_pos + j * ch->ca_rate;
            uint64_t E = P + (1ull << 31), L;
            if (E >= FULL) E -= FULL;
            L = P >= (1ull << 31) ? P - (1ull << 31) : P + FULL - (1ull << 31);
            const uint64_t pos[3] = {E, P, L};
            for (int k = 0; k < 3; ++k) {
                const int h = 1 - 2 * chip_at(chips, pos[k]);
                I[k] += h * (vi * C - vq * S);
                Q[k] += h * (vi * S + vq * C);
            }
        }
        const int32_t IE = (int32_t)I[0], QE = (int32_t)Q[0], IP = (int32_t)I[1], QP = (int32_t)Q[1], IL = (int32_t)I[2], QL = (int32_t)Q[2];
        if (prompt) {
            prompt[2 * t] = IP;
            prompt[2 * t + 1] = QP;
        }
        if (records) {
            gpsacq_track_record *r = &records[t];
            r->sample = ch->next_sample;
            r->ie = IE; r->qe = QE; r->ip = IP; r->qp = QP; r->il = IL; r->ql = QL;
            r->lo_rate = ch->lo_rate;
            r->ca_rate = ch->ca_rate;
        }
        ch->lo_phase += (uint32_t)n * ch->lo_rate;
        ch->ca_pos = ch->ca_pos + n * ch->ca_rate - FULL;
        ch->next_sample += n;
        ch->epoch += 1;
        ++t;
        const int k = ch->epoch;
        if (p->agc_period > 0 && k % p->agc_period == 0) {
            int64_t S = 0;
            ch->pwr[ch->pwr_pos] = (int64_t)IP * IP + (int64_t)QP * QP;
            ch->pwr_pos = (ch->pwr_pos + 1) % 8;
            for (int i = 0; i < 8; ++i) S += ch->pwr[i];
            if (ch->gain_adj != 0) {
                if (S < 8 * p->agc_lo) ch->gain_adj = 0;
            } else if (S > 8 * p->agc_hi) {
                ch->gain_adj = -1;
            }
        }
        if (ch->fll_left > 0) {
            const int64_t dot = (int64_t)ch->prev_ip * IP + (int64_t)ch->prev_qp * QP;
            const int64_t cross = (int64_t)ch->prev_ip * QP - (int64_t)ch->prev_qp * IP;
            const int64_t e = (dot > 0) - (dot < 0);
            lo_int += (uint64_t)(e * cross) * (1ull << p->fll_k);
            ch->lo_rate = (uint32_t)(lo_int >> 32);
            ch->fll_left -= 1;
        } else {
            const int64_t e = (int64_t)IP * QP;
            lo_int += (uint64_t)e * (1ull << (p->lo_ki + ch->gain_adj));
            ch->lo_rate = (uint32_t)((lo_int + (uint64_t)e * (1ull << (p->lo_kp + ch->gain_adj))) >> 32);
        }
        ch->prev_ip = IP;
        ch->prev_qp = QP;
        {
            const int64_t e = ((int64_t)IE * IE + (int64_t)QE * QE) - ((int64_t)IL * IL + (int64_t)QL * QL);
            ca_int += (uint64_t)e * (1ull << p->ca_ki);
            ch->ca_rate = (uint32_t)((ca_int + (uint64_t)e * (1ull << p->ca_kp)) >> 32);
        }
        if (k == p->aid_epoch) {
            lo_int = lo_nom + (ca_int - ca_nom) * 1540ull;
            ch->lo_rate = (uint32_t)(lo_int >> 32);
        }
        if (out_of(lo_int, lo_nom, p->lo_window) || out_of((uint64_t)ch->lo_rate << 32, lo_nom, p->lo_window) ||
            out_of(ca_int, ca_nom, p->ca_window) || out_of((uint64_t)ch->ca_rate << 32, ca_nom, p->ca_window))
            ch->status = GPSACQ_TRACK_LOST;
    }
    ch->lo_int = (int64_t)lo_int;
    ch->ca_int = (int64_t)ca_int;
    return t;
}
