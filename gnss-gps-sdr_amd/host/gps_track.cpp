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
// and, when at least four channels have a valid ephemeris (subframes 1-3) and a time tag, one position fix per second of capture
// (gpsacq_observables + gpsacq_fix_batch), from the first whole second at which every such channel has records to the last:
//     fix tow T lat LAT lon LON alt ALT n_used N rms R          (T seconds of week, degrees, metres)
// With GPSACQ_VELOCITY=1 in the environment every fix whose velocity could be solved (gpsacq_rate_observables over half a second of
// samples centred on the instant + gpsacq_vel_batch) is followed by a second line; without it the output is unchanged:
//     vel tow T ve E vn N vu U drift D n_used N rms R           (m/s east, north, up; drift of the sampling clock, parts in 1)
// With GPSACQ_SMOOTH_MS=W (1 .. 65536) the fixes are made from carrier-smoothed observations (gpsacq_smooth_observables): instants
// a thousandth of a second of samples apart from the first record every channel has, a window of W instants, the fix of every
// 1000th instant -- the same once-a-second instants -- in the same format, and after the fixes one line per channel with the
// scatter of the code against the carrier over the full windows (the measured pseudorange sigma, metres):
//     sigma PRN P code_sigma_m S full N
// With GPSACQ_QUALITY=1 every whole second of the capture at which a channel has records gets one line with the C/N0 estimate of
// every such channel (gpsacq_quality_observables at its default parameters: dB-Hz over the last 200 epochs, the flags
// GPSACQ_QUALITY_* as a number), printed after the channels' own lines, and the fixes are made from observations that carry the
// weights of that estimate (a channel below 30 dB-Hz or out of phase lock has none); without it the output is unchanged:
//     cn0 sec K PRN P dbhz X flags F [PRN P dbhz X flags F ...]
//
// With GPSACQ_INPUT=iq_u8|iq_s8 in the environment FILE is an 8-bit IQ capture (rtl-sdr / HackRF, README.md:83-115), read the way
// gps_test reads it (host/search_api.cpp: GPSACQ_MIX_HZ, GPSACQ_IQ_KEEP_DC, GPSACQ_IQ_MULTIBIT, GPSACQ_IQ_COMPLEX; the mean of the
// whole capture): searched with gpsacq_search_iq8, channels from gpsacq_track_start_iq8, tracked with gpsacq_track_iq8 -- as 1-bit
// channels on the converted stream, or with GPSACQ_IQ_MULTIBIT / GPSACQ_IQ_COMPLEX as multi-bit complex channels whose loop
// settings come from the capture's RMS (gpsacq_track_default_params_iq8).  Same output lines.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gpsacq.h"

static int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

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
    // input format: the environment gps_test honours
    const char* fmt = std::getenv("GPSACQ_INPUT");
    bool iq = false;
    gpsacq_iq8_input iqin;
    std::memset(&iqin, 0, sizeof iqin);
    if (fmt && *fmt && std::strcmp(fmt, "bits") != 0) {
        if (std::strcmp(fmt, "iq_u8") == 0) iqin.format = GPSACQ_IQ_U8;
        else if (std::strcmp(fmt, "iq_s8") == 0) iqin.format = GPSACQ_IQ_S8;
        else {
            std::fprintf(stderr, "gps_track: GPSACQ_INPUT=%s is not one of bits, iq_u8, iq_s8\n", fmt);
            std::fclose(fp);
            return 64;
        }
        iq = true;
        const char* mix = std::getenv("GPSACQ_MIX_HZ");
        iqin.mix_hz = (mix && *mix) ? std::atof(mix) : 0.0;
        iqin.fs = prm.fs;
        iqin.remove_dc = env_int("GPSACQ_IQ_KEEP_DC", 0) ? 0 : 1;
        iqin.multibit = env_int("GPSACQ_IQ_COMPLEX", 0) ? GPSACQ_SAMPLES_COMPLEX : env_int("GPSACQ_IQ_MULTIBIT", 0) ? GPSACQ_SAMPLES_REAL : GPSACQ_SAMPLES_SIGN;
    }
    const size_t block_bytes = iq ? (size_t)GPSACQ_BLOCK_BYTES * 16 : (size_t)GPSACQ_BLOCK_BYTES;  // one Sample(): 40960 samples
    std::fseek(fp, 0, SEEK_END);
    size_t n_bytes = (size_t)std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    if (iq) {
        n_bytes &= ~(size_t)1;
        if (secs > 0 && (size_t)(secs * prm.fs) * 2 < n_bytes) n_bytes = (size_t)(secs * prm.fs) * 2;
    } else if (secs > 0 && (size_t)(secs * prm.fs / 8) < n_bytes) n_bytes = (size_t)(secs * prm.fs / 8);
    std::vector<uint8_t> bits(n_bytes);
    n_bytes = std::fread(bits.data(), 1, n_bytes, fp);
    std::fclose(fp);
    if (iq) n_bytes &= ~(size_t)1;
    const size_t n_samples = iq ? n_bytes / 2 : n_bytes * 8;
    const size_t n_blocks = n_bytes / block_bytes < GPSACQ_NUM_SATS ? n_bytes / block_bytes : GPSACQ_NUM_SATS;
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
    gpsacq_track_params tp;
    const gpsacq_track_params* params = nullptr;  // the defaults, except for multi-bit channels
    if (iq) {
        // `y = y - mean(y)` is the mean of the capture (proc_rtl_bin_for_gps.m:17); multi-bit loops are set from its RMS
        iqin.total_samples = n_samples;
        int64_t sums[2] = {0, 0};
        uint64_t power[2] = {0, 0};
        const size_t chunk = (size_t)1 << 24;
        for (size_t s0 = 0; rc == 0 && s0 < n_samples; s0 += chunk) {
            const size_t m = n_samples - s0 < chunk ? n_samples - s0 : chunk;
            if (iqin.remove_dc) rc = gpsacq_iq8_accumulate_sums(e, bits.data() + 2 * s0, m, iqin.format, sums);
            if (rc == 0 && iqin.multibit) rc = gpsacq_iq8_accumulate_power(e, bits.data() + 2 * s0, m, iqin.format, power);
        }
        iqin.mean_i = (double)sums[0] / (double)n_samples;
        iqin.mean_q = (double)sums[1] / (double)n_samples;
        if (rc == 0 && iqin.multibit) {
            // RMS of v = a - dc:  E[a^2] - 2 dc E[a] + dc^2 per arm
            const double di = iqin.remove_dc ? std::nearbyint(iqin.mean_i) : 0.0, dq = iqin.remove_dc ? std::nearbyint(iqin.mean_q) : 0.0;
            const double msq = ((double)power[0] + (double)power[1]) / (double)n_samples - 2 * di * iqin.mean_i - 2 * dq * iqin.mean_q + di * di + dq * dq;
            rc = gpsacq_track_default_params_iq8(e, std::sqrt(msq > 0 ? msq / 2 : 0.0), &tp);
            params = &tp;
        }
        if (rc == 0) rc = gpsacq_search_iq8(e, &iqin, bits.data(), n_blocks, block_bytes, nullptr, n_blocks, nullptr, peaks.data());
    } else {
        rc = gpsacq_search(e, bits.data(), n_blocks, GPSACQ_BLOCK_BYTES, nullptr, n_blocks, nullptr, peaks.data());
    }
    std::vector<gpsacq_track_chan> chans;
    for (size_t b = 0; rc == 0 && b < n_blocks; ++b) {
        if (!(peaks[b].snr > 25.0f)) continue;
        gpsacq_track_chan ch;
        const uint64_t block_first = (uint64_t)b * GPSACQ_BLOCK_BYTES * 8;
        rc = iq ? gpsacq_track_start_iq8(e, &iqin, (int)(b % 32) + 1, &peaks[b], block_first, params, &ch)
                : gpsacq_track_start(e, (int)(b % 32) + 1, &peaks[b], block_first, nullptr, &ch);
        chans.push_back(ch);
    }
    gpsacq_info info;
    gpsacq_get_info(e, &info);
    const int max_epochs = (int)(n_samples / (size_t)info.num_lags) + 2;
    std::vector<int32_t> prompt(chans.size() * (size_t)max_epochs * 2), n_ep(chans.size());
    std::vector<gpsacq_track_record> records(chans.size() * (size_t)max_epochs);
    if (rc == 0 && !chans.empty())
        rc = iq ? gpsacq_track_iq8(e, &iqin, bits.data(), n_samples, 0, chans.data(), (int)chans.size(), params, prompt.data(), records.data(), max_epochs, n_ep.data())
                : gpsacq_track(e, bits.data(), n_bytes, 0, chans.data(), (int)chans.size(), nullptr, prompt.data(), records.data(), max_epochs, n_ep.data());
    if (rc) {
        std::fprintf(stderr, "gps_track: %d: %s\n", rc, gpsacq_last_error());
        gpsacq_destroy(e);
        return rc;
    }
    const double two32 = 4294967296.0;
    // the channels a fix can use: their ephemerides, time tags and rows of `records`
    std::vector<gpsacq_ephemeris> ephs;
    std::vector<gpsacq_time_tag> tags;
    std::vector<size_t> fix_chan;
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
        // Doppler: the carrier word against the IF -- fc, or for a multi-bit channel the signed word against the satellite-free
        // carrier of the raw capture, fc - mix_hz (complex baseband: -mix_hz)
        const double dop_hz = iq && iqin.multibit
                                  ? (int32_t)ch.lo_rate / two32 * prm.fs - ((iqin.multibit == GPSACQ_SAMPLES_COMPLEX ? 0.0 : prm.fc) - iqin.mix_hz)
                                  : ch.lo_rate / two32 * prm.fs - prm.fc;
        std::printf("chan %zu PRN %d status %s epochs %d dop_hz %.1f code_hz %.3f bits %d\n", c, ch.prn, ch.status ? "lost" : "ok", n,
                    dop_hz, ch.ca_rate / two32 * prm.fs, n_bits);
        std::vector<gpsacq_subframe> sf(n_bits / 300 + 1);
        int n_sf = 0, n_fail = 0;
        gpsacq_nav_subframes(nb.data(), n_bits, sf.data(), (int)sf.size(), &n_sf, &n_fail);
        for (int k = 0; k < n_sf && k < (int)sf.size(); ++k) std::printf("subframe PRN %d id %d tow %d\n", ch.prn, sf[k].id, sf[k].tow);
        std::printf("parity PRN %d failures %d\n", ch.prn, n_fail);
        if (n_sf > (int)sf.size()) n_sf = (int)sf.size();
        gpsacq_ephemeris eph;
        std::memset(&eph, 0, sizeof eph);
        eph.prn = ch.prn;
        gpsacq_time_tag tag;
        if (n_sf > 0 && fix_chan.size() < GPSACQ_FIX_MAX_SATS && gpsacq_ephemeris_load(&eph, sf.data(), n_sf) == GPSACQ_OK &&
            gpsacq_ephemeris_valid(&eph) && gpsacq_time_tag_from_subframe(&sf[0], e0, (int)ephs.size(), &tag) == GPSACQ_OK) {
            ephs.push_back(eph);
            tags.push_back(tag);
            fix_chan.push_back(c);
        }
    }
    const bool want_quality = env_int("GPSACQ_QUALITY", 0) != 0;
    const uint64_t second = (uint64_t)std::llround(prm.fs);
    if (want_quality && !chans.empty() && second > 0 && n_samples > second) {
        // the estimate needs no time tag beyond `valid`: every channel, twelve to a call, at the whole seconds inside the capture
        const size_t n_sec = (size_t)((n_samples - 1) / second);
        std::vector<gpsacq_quality_info> qi(n_sec * chans.size()), part(n_sec * GPSACQ_FIX_MAX_SATS);
        gpsacq_time_tag any[GPSACQ_FIX_MAX_SATS];
        std::memset(any, 0, sizeof any);
        for (auto& t : any) t.valid = 1;
        for (size_t g0 = 0; rc == 0 && g0 < chans.size(); g0 += GPSACQ_FIX_MAX_SATS) {
            const size_t ng = chans.size() - g0 < GPSACQ_FIX_MAX_SATS ? chans.size() - g0 : GPSACQ_FIX_MAX_SATS;
            rc = gpsacq_quality_observables(e, records.data() + g0 * (size_t)max_epochs, max_epochs, n_ep.data() + g0, chans.data() + g0, any, (int)ng,
                                            second, second, n_sec, nullptr, nullptr, part.data());
            for (size_t k = 0; rc == 0 && k < n_sec; ++k)
                for (size_t c = 0; c < ng; ++c) qi[k * chans.size() + g0 + c] = part[k * ng + c];
        }
        if (rc) {
            std::fprintf(stderr, "gps_track: %d: %s\n", rc, gpsacq_last_error());
            gpsacq_destroy(e);
            return rc;
        }
        for (size_t k = 0; k < n_sec; ++k) {
            bool head = false;
            for (size_t c = 0; c < chans.size(); ++c) {
                const gpsacq_quality_info& q = qi[k * chans.size() + c];
                if (q.epochs == 0) continue;
                if (!head) std::printf("cn0 sec %zu", k + 1);
                head = true;
                std::printf(" PRN %d dbhz %.2f flags %d", chans[c].prn, q.cn0_dbhz, q.flags);
            }
            if (head) std::printf("\n");
        }
    }
    if (fix_chan.size() >= 4) {
        const size_t m = fix_chan.size();
        std::vector<gpsacq_track_record> rec(m * (size_t)max_epochs);
        std::vector<gpsacq_track_chan> fch(m);
        std::vector<int32_t> fn(m);
        uint64_t from = 0, to = UINT64_MAX;  // every channel has records over [from, to)
        for (size_t k = 0; k < m; ++k) {
            const size_t c = fix_chan[k];
            std::memcpy(&rec[k * max_epochs], &records[c * max_epochs], (size_t)n_ep[c] * sizeof(gpsacq_track_record));
            fch[k] = chans[c];
            fn[k] = n_ep[c];
            const uint64_t first = n_ep[c] > 0 ? records[c * max_epochs].sample : chans[c].next_sample;
            if (first > from) from = first;
            if (chans[c].next_sample < to) to = chans[c].next_sample;
        }
        const uint64_t step = (uint64_t)std::llround(prm.fs);  // one second of samples
        const uint64_t first_rx = (from + step - 1) / step * step;
        if (step > 0 && first_rx < to) {
            const size_t n_fix = (size_t)((to - 1 - first_rx) / step) + 1;
            std::vector<gpsacq_obs> obs(n_fix * m);
            std::vector<gpsacq_fix> fix(n_fix);
            // the word of zero Doppler: what lo_nom holds, except for multi-bit channels, which keep their start word there
            std::vector<uint32_t> nom(m);
            uint32_t iq_word = 0;
            const bool want_vel = env_int("GPSACQ_VELOCITY", 0) != 0;
            const int smooth_ms = env_int("GPSACQ_SMOOTH_MS", 0);
            if (iq && iqin.multibit && (want_vel || smooth_ms > 0)) rc = gpsacq_track_nominal_word_iq8(e, &iqin, &iq_word);
            for (size_t k = 0; k < m; ++k) nom[k] = iq && iqin.multibit ? iq_word : (uint32_t)((uint64_t)fch[k].lo_nom >> 32);
            const uint64_t ms_step = step / 1000;
            std::vector<gpsacq_smooth_info> sinfo;
            size_t n_ms = 0;
            if (rc == 0 && smooth_ms > 0 && ms_step > 0) {
                // instants a millisecond apart that hit every whole second: back from the first one to the start of the records
                const uint64_t back = (first_rx - from) / ms_step;
                const uint64_t start = first_rx - back * ms_step;
                n_ms = (size_t)((to - 1 - start) / ms_step) + 1;
                gpsacq_smooth_params sp;
                gpsacq_smooth_default_params(&sp);
                sp.window = smooth_ms;
                std::vector<gpsacq_obs> sobs(n_ms * m);
                sinfo.resize(n_ms * m);
                rc = gpsacq_smooth_observables(e, rec.data(), max_epochs, fn.data(), fch.data(), tags.data(), nom.data(), (int)m, start, ms_step, n_ms,
                                               &sp, sobs.data(), sinfo.data());
                for (size_t k = 0; rc == 0 && k < n_fix; ++k) {
                    const size_t i = (size_t)back + k * 1000;
                    if (i < n_ms) std::memcpy(&obs[k * m], &sobs[i * m], m * sizeof(gpsacq_obs));
                    else std::memset(&obs[k * m], 0, m * sizeof(gpsacq_obs));
                }
            } else if (rc == 0) {
                rc = gpsacq_observables(e, rec.data(), max_epochs, fn.data(), fch.data(), tags.data(), (int)m, first_rx, step, n_fix, obs.data());
            }
            if (rc == 0 && want_quality) {
                // the weights of the same instants into the observations: smoothed ones lie 1000 millisecond steps apart
                std::vector<gpsacq_quality_info> qinfo(n_fix * m);
                rc = gpsacq_quality_observables(e, rec.data(), max_epochs, fn.data(), fch.data(), tags.data(), (int)m, first_rx,
                                                n_ms > 0 ? 1000 * ms_step : step, n_fix, nullptr, obs.data(), qinfo.data());
            }
            if (rc == 0) rc = gpsacq_fix_batch(e, ephs.data(), (int)ephs.size(), obs.data(), n_fix, (int)m, fix.data());
            if (rc) {
                std::fprintf(stderr, "gps_track: %d: %s\n", rc, gpsacq_last_error());
                gpsacq_destroy(e);
                return rc;
            }
            std::vector<gpsacq_vel> vel;
            if (want_vel) {
                std::vector<gpsacq_rate_obs> robs(n_fix * m);
                vel.resize(n_fix);
                if (rc == 0)
                    rc = gpsacq_rate_observables(e, rec.data(), max_epochs, fn.data(), fch.data(), nom.data(), (int)m, first_rx, step, n_fix,
                                                 step / 2 > 0 ? step / 2 : 1, robs.data());
                if (rc == 0) rc = gpsacq_vel_batch(e, ephs.data(), (int)ephs.size(), obs.data(), robs.data(), fix.data(), n_fix, (int)m, vel.data());
                if (rc) {
                    std::fprintf(stderr, "gps_track: %d: %s\n", rc, gpsacq_last_error());
                    gpsacq_destroy(e);
                    return rc;
                }
            }
            const double deg = 180.0 / 3.14159265358979323846;
            for (size_t k = 0; k < n_fix; ++k)
                if (fix[k].status == GPSACQ_FIX_OK) {
                    std::printf("fix tow %.6f lat %.7f lon %.7f alt %.2f n_used %d rms %.2f\n", fix[k].rx_ms * 1e-3 + fix[k].rx_frac,
                                fix[k].lat * deg, fix[k].lon * deg, fix[k].alt, fix[k].n_used, fix[k].rms);
                    if (want_vel && vel[k].status == GPSACQ_VEL_OK)
                        std::printf("vel tow %.6f ve %.3f vn %.3f vu %.3f drift %.4e n_used %d rms %.3f\n", fix[k].rx_ms * 1e-3 + fix[k].rx_frac,
                                    vel[k].ve, vel[k].vn, vel[k].vu, vel[k].drift, vel[k].n_used, vel[k].rms);
                }
            for (size_t k = 0; n_ms > 0 && k < m; ++k) {
                // corr is in cycles * 2^32: times the L1 wavelength it is the code's distance from its carrier-held mean
                const double unit = 299792458.0 / 1575.42e6 / two32;
                double sum = 0.0, sq = 0.0;
                size_t full = 0;
                for (size_t i = 0; i < n_ms; ++i)
                    if (sinfo[i * m + k].flags & GPSACQ_SMOOTH_FULL) {
                        const double v = (double)sinfo[i * m + k].corr * unit;
                        sum += v, sq += v * v, ++full;
                    }
                const double var = full ? sq / (double)full - (sum / (double)full) * (sum / (double)full) : 0.0;
                std::printf("sigma PRN %d code_sigma_m %.3f full %zu\n", fch[k].prn, std::sqrt(var > 0 ? var : 0.0), full);
            }
        }
    }
    gpsacq_destroy(e);
    return 0;
}
