// gpsacq_track.cpp -- host side of "Tracking channels and NAV data" of include/gpsacq.h.  First the channels: default loop
// parameters, a channel's start from a search hit, and the gpsacq_track* entry points that run track_kernels.hip (1-bit stream)
// or track_iq_kernels.hip (8-bit IQ capture) on the engine of gpsacq_engine.hpp.  Then the NAV decoder, host only: bit sync and
// NAV bits from the prompt I arm, and the subframe scan of CHANNEL::ParityCheck() (c/channel.cpp:329-353) with the parity equations
// of IS-GPS-200 Table 20-XIV.
// Compiled with -ffp-contract=off like gpsacq_engine.cpp: the default parameters and NCO words are host floating point that tests pin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "acq_tables.hpp"
#include "gpsacq_engine.hpp"
#include "track_launch.hpp"

using namespace acq;

// ---- tracking channels (track_channel.hpp, track_kernels.hip; the model is in include/gpsacq.h) ---------------------------
extern "C" int gpsacq_track_default_params(const gpsacq_engine* e, gpsacq_track_params* p) {
    if (!e || !p) return fail(GPSACQ_ERR_ARG, "gpsacq_track_default_params: null argument");
    // above 40 MHz num_lags saturates at N_FFT = 40000 and is no longer samples per millisecond: no defaults can be built from it
    if (e->p.fs > 40.0e6) return fail(GPSACQ_ERR_UNSUPPORTED, "gpsacq_track_default_params: fs %.0f Hz is above 40 MHz", e->p.fs);
    const double fs = e->p.fs, r = (double)e->nlags / 10000.0;
    // round(log2((10000 / spm)^2)) up to 10 MHz; above it round(log2((10000 / spm)^3)): a step of the NCO word is worth fs / 2^32 Hz,
    // so with the square rule the loops' bandwidth in Hz grows with fs (at 40 MHz the Costas loop no longer holds the phase)
    const double octaves = std::log2(10000.0 / e->nlags);
    const int adj = (int)std::lround((e->nlags > 10000 ? 3.0 : 2.0) * octaves);
    p->lo_ki = 20 + adj;
    p->lo_kp = 27 + adj;
    p->ca_ki = 11 + adj;
    p->ca_kp = 23 + adj;
    p->fll_k = 25 + adj;
    p->fll_epochs = 500;
    p->aid_epoch = -1;
    p->agc_period = 250;
    p->agc_lo = (int64_t)std::floor(1200.0 * 1200.0 * r * r);
    p->agc_hi = (int64_t)std::floor(1400.0 * 1400.0 * r * r);
    const double two64 = 4294967296.0 * 4294967296.0;
    p->lo_window = (int64_t)(10000.0 / fs * two64);
    p->ca_window = (int64_t)(4.0 * 10000.0 / 1540.0 / fs * two64);
    p->min_epoch = e->nlags / 2;
    p->max_epoch = std::min(2 * e->nlags, 65535);  // the kernel packs two counts <= max_epoch per 32-bit word
    return GPSACQ_OK;
}

extern "C" int gpsacq_track_start(const gpsacq_engine* e, int prn, const gpsacq_peak* peak, uint64_t block_first_sample,
                                  const gpsacq_track_params* params, gpsacq_track_chan* ch) {
    if (!e || !peak || !ch || prn < 1 || prn > GPSACQ_NUM_SATS) return fail(GPSACQ_ERR_ARG, "gpsacq_track_start: bad argument");
    gpsacq_track_params p;
    if (params) p = *params;
    else if (int rc = gpsacq_track_default_params(e, &p)) return rc;
    gpsacq_handoff_t h;
    if (int rc = gpsacq_handoff_engine(e, peak, 0.0, &h)) return rc;
    if (peak->ca_shift < 0 || h.ca_rate == 0) return fail(GPSACQ_ERR_ARG, "gpsacq_track_start: bad hit (ca_shift %d)", peak->ca_shift);
    const uint64_t full = 1023ull << 32;
    std::memset(ch, 0, sizeof *ch);
    ch->prn = prn;
    ch->status = GPSACQ_TRACK_OK;
    ch->lo_rate = h.lo_rate;
    ch->ca_rate = h.ca_rate;
    ch->lo_int = (int64_t)((uint64_t)h.lo_rate << 32);
    ch->ca_int = (int64_t)((uint64_t)h.ca_rate << 32);
    ch->lo_nom = (int64_t)((uint64_t)(uint32_t)(e->p.fc / e->p.fs * 4294967296.0) << 32);
    ch->ca_nom = (int64_t)((uint64_t)(uint32_t)(1.023e6 / e->p.fs * 4294967296.0) << 32);
    ch->fll_left = p.fll_epochs;
    // the prompt position at block_first_sample is ca_shift samples of the code NCO; then the pause to the next code epoch
    const uint64_t pos = ((uint64_t)peak->ca_shift * h.ca_rate) % full;
    const uint64_t n0 = (full - pos + h.ca_rate - 1) / h.ca_rate;
    ch->next_sample = block_first_sample + n0;
    ch->lo_phase = (uint32_t)((block_first_sample + n0) * (uint64_t)h.lo_rate);
    ch->ca_pos = pos + n0 * h.ca_rate - full;
    return GPSACQ_OK;
}

static int track_check_params(const gpsacq_track_params& p) {
    const int sh[] = {p.lo_ki - 1, p.lo_kp - 1, p.ca_ki, p.ca_kp, p.fll_k};  // the carrier shifts must stay >= 0 with gain_adj = -1
    for (int v : sh)
        if (v < 0 || v > 62) return fail(GPSACQ_ERR_ARG, "gpsacq_track: a loop shift is outside [0, 62] (lo_ki/lo_kp >= 1)");
    if (p.min_epoch < 1 || p.max_epoch < p.min_epoch || p.max_epoch > 65535 || p.lo_window < 0 || p.ca_window < 0)
        return fail(GPSACQ_ERR_ARG, "gpsacq_track: need 1 <= min_epoch <= max_epoch <= 65535 and windows >= 0");
    return GPSACQ_OK;
}

// the C/A chip table of the channels (and of the 8-bit IQ generator), built on first use
int ensure_track_chips(gpsacq_engine* e) {
    if (e->d_track_chips) return GPSACQ_OK;
    const std::vector<uint32_t> chips = ca_chip_words();
    HIPCHK(e->d_track_chips.alloc(chips.size()));
    HIPCHK(hipMemcpy(e->d_track_chips, chips.data(), chips.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return GPSACQ_OK;
}

// what every gpsacq_track* call does before its kernel: the channel states are checked and uploaded to e->d_chans ...
static int track_prepare(gpsacq_engine* e, uint64_t first_sample, const gpsacq_track_chan* chans, int n_chans) {
    for (int c = 0; c < n_chans; ++c) {
        const gpsacq_track_chan& ch = chans[c];
        if (ch.prn < 1 || ch.prn > GPSACQ_NUM_SATS || ch.ca_rate == 0 || ch.ca_pos >= (1023ull << 32) || ch.pwr_pos < 0 || ch.pwr_pos > 7)
            return fail(GPSACQ_ERR_ARG, "gpsacq_track: channel %d is not a valid state", c);
        if (ch.next_sample < first_sample)
            return fail(GPSACQ_ERR_ARG, "gpsacq_track: channel %d continues at sample %llu, before the window's first sample %llu", c,
                        (unsigned long long)ch.next_sample, (unsigned long long)first_sample);
    }
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = ensure_track_chips(e)) return rc;
    if (int rc = e->d_chans.grow((size_t)n_chans, e->stream)) return rc;
    if (int rc = e->d_track_n.grow((size_t)n_chans, e->stream)) return rc;
    HIPCHK(hipMemcpyAsync(e->d_chans, chans, n_chans * sizeof(gpsacq_track_chan), hipMemcpyHostToDevice, e->stream));
    return GPSACQ_OK;
}
// ... and after it: states and epoch counts back, wait
static int track_collect(gpsacq_engine* e, gpsacq_track_chan* chans, int n_chans, int32_t* n_epochs_out) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(chans, e->d_chans, n_chans * sizeof(gpsacq_track_chan), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(n_epochs_out, e->d_track_n, n_chans * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}
// the part of a kernel's arguments that does not depend on the sample format
static void track_common(const gpsacq_engine* e, uint64_t first_sample, uint64_t n_samples, int n_chans, const gpsacq_track_params& p, void* d_prompt,
                         void* d_records, int max_epochs, TrackCommon& a) {
    a.first_sample = first_sample;
    a.n_samples = n_samples;
    a.chans = e->d_chans;
    a.n_chans = n_chans;
    a.prm = p;
    a.chips = e->d_track_chips;
    a.prompt = (int32_t*)d_prompt;
    a.records = (gpsacq_track_record*)d_records;
    a.max_epochs = max_epochs;
    a.n_epochs = e->d_track_n;
}
static void track_launch_bits(gpsacq_engine* e, const void* d_bits, size_t n_bytes, uint64_t first_sample, int n_chans, const gpsacq_track_params& p,
                              void* d_prompt, void* d_records, int max_epochs) {
    TrackArgs a{};
    track_common(e, first_sample, 8ull * n_bytes, n_chans, p, d_prompt, d_records, max_epochs, a);
    a.bits = (const uint8_t*)d_bits;
    a.n_bytes = n_bytes;
    launch_track(a, e->stream);
}

extern "C" int gpsacq_track_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, uint64_t first_sample, gpsacq_track_chan* chans,
                                   int n_chans, const gpsacq_track_params* params, void* d_prompt, void* d_records, int max_epochs,
                                   int32_t* n_epochs_out) {
    if (!e || !d_bits || !chans || n_chans <= 0 || max_epochs < 0 || !n_epochs_out)
        return fail(GPSACQ_ERR_ARG, "gpsacq_track: bad argument");
    if (((uintptr_t)d_bits & 3) || (first_sample & 7)) return fail(GPSACQ_ERR_ARG, "gpsacq_track: bits must be 4-byte aligned, first_sample a multiple of 8");
    gpsacq_track_params p;
    if (params) p = *params;
    else if (int rc = gpsacq_track_default_params(e, &p)) return rc;
    if (int rc = track_check_params(p)) return rc;
    if (int rc = track_prepare(e, first_sample, chans, n_chans)) return rc;
    track_launch_bits(e, d_bits, n_bytes, first_sample, n_chans, p, d_prompt, d_records, max_epochs);
    return track_collect(e, chans, n_chans, n_epochs_out);
}

// only the epochs each channel ran are defined; copy them row by row
static int track_rows_to_host(gpsacq_engine* e, int n_chans, int max_epochs, const int32_t* n_epochs, int32_t* prompt, gpsacq_track_record* records) {
    for (int c = 0; c < n_chans; ++c) {
        const size_t ne = (size_t)n_epochs[c], r = (size_t)c * max_epochs;
        if (!ne) continue;
        if (prompt) HIPCHK(hipMemcpyAsync(prompt + 2 * r, e->d_prompt + 2 * r, 2 * ne * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        if (records) HIPCHK(hipMemcpyAsync(records + r, e->d_records + r, ne * sizeof(gpsacq_track_record), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}
// what the host-buffer entry points do once their window is uploaded: prompt / record scratch, the device entry point (run, given
// the two scratch pointers), the rows back
template <class Run> static int track_from_host(gpsacq_engine* e, int n_chans, int max_epochs, int32_t* prompt, gpsacq_track_record* records,
                                                const int32_t* n_epochs, Run run) {
    const size_t per = (size_t)n_chans * (size_t)max_epochs;
    if (prompt && per)
        if (int rc = e->d_prompt.grow(2 * per, e->stream)) return rc;
    if (records && per)
        if (int rc = e->d_records.grow(per, e->stream)) return rc;
    if (int rc = run(prompt && per ? (void*)e->d_prompt : nullptr, records && per ? (void*)e->d_records : nullptr)) return rc;
    return track_rows_to_host(e, n_chans, max_epochs, n_epochs, prompt, records);
}

extern "C" int gpsacq_track(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, uint64_t first_sample, gpsacq_track_chan* chans,
                            int n_chans, const gpsacq_track_params* params, int32_t* prompt, gpsacq_track_record* records,
                            int max_epochs, int32_t* n_epochs_out) {
    if (!e || !bits || n_bytes == 0 || !chans || n_chans <= 0 || max_epochs < 0 || !n_epochs_out)
        return fail(GPSACQ_ERR_ARG, "gpsacq_track: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_gen.grow(n_bytes, e->stream)) return rc;
    HIPCHK(hipMemcpyAsync(e->d_gen, bits, n_bytes, hipMemcpyHostToDevice, e->stream));
    return track_from_host(e, n_chans, max_epochs, prompt, records, n_epochs_out, [&](void* d_prompt, void* d_records) {
        return gpsacq_track_device(e, e->d_gen, n_bytes, first_sample, chans, n_chans, params, d_prompt, d_records, max_epochs, n_epochs_out);
    });
}

// ---- tracking channels on an 8-bit IQ capture (track_iq_kernels.hip; include/gpsacq.h) -------------------------------------
extern "C" int gpsacq_track_default_params_iq8(const gpsacq_engine* e, double sample_rms, gpsacq_track_params* params) {
    if (!e || !params) return fail(GPSACQ_ERR_ARG, "gpsacq_track_default_params_iq8: null argument");
    if (!(sample_rms > 0) || !std::isfinite(sample_rms)) return fail(GPSACQ_ERR_UNSUPPORTED, "gpsacq_track_default_params_iq8: sample_rms %g", sample_rms);
    gpsacq_track_params q;  // *params is written only on success
    gpsacq_track_params* p = &q;
    if (int rc = gpsacq_track_default_params(e, p)) return rc;
    int g = (int)std::lround(std::log2((double)GPSACQ_TRACK_IQ8_GAIN * sample_rms * sample_rms));
    // every shift stays in [0, 62], the carrier's in [1, 62] (gain_adj = -1)
    const int lo = std::min(std::min(p->lo_ki, p->lo_kp) - 1, std::min(std::min(p->ca_ki, p->ca_kp), p->fll_k));
    const int hi = std::max(std::max(p->lo_ki, p->lo_kp), std::max(std::max(p->ca_ki, p->ca_kp), p->fll_k));
    g = std::max(g, hi - 62);
    if (g > lo) return fail(GPSACQ_ERR_UNSUPPORTED, "gpsacq_track_default_params_iq8: sample_rms %g needs shifts below 0", sample_rms);
    p->lo_ki -= g, p->lo_kp -= g, p->ca_ki -= g, p->ca_kp -= g, p->fll_k -= g;
    const double s = std::ldexp(1.0, g);
    p->agc_lo = (int64_t)std::floor((double)p->agc_lo * s);
    p->agc_hi = (int64_t)std::floor((double)p->agc_hi * s);
    *params = q;
    return GPSACQ_OK;
}

extern "C" int gpsacq_iq8_accumulate_power(const gpsacq_engine* e, const void* iq, size_t n_samples, int format, uint64_t power[2]) {
    (void)e;  // host arithmetic: no device, the engine may be NULL
    if (!iq || !power || n_samples == 0) return fail(GPSACQ_ERR_ARG, "gpsacq_iq8_accumulate_power: bad argument");
    if (format != GPSACQ_IQ_U8 && format != GPSACQ_IQ_S8) return fail(GPSACQ_ERR_ARG, "unknown IQ format %d", format);
    const uint8_t* b = (const uint8_t*)iq;
    uint64_t pi = 0, pq = 0;
    for (size_t s = 0; s < n_samples; ++s) {
        const int vi = format == GPSACQ_IQ_S8 ? (int)(int8_t)b[2 * s] : (int)b[2 * s] - 128;
        const int vq = format == GPSACQ_IQ_S8 ? (int)(int8_t)b[2 * s + 1] : (int)b[2 * s + 1] - 128;
        pi += (uint64_t)(vi * vi);
        pq += (uint64_t)(vq * vq);
    }
    power[0] += pi;
    power[1] += pq;
    return GPSACQ_OK;
}

extern "C" int gpsacq_track_start_iq8(const gpsacq_engine* e, const gpsacq_iq8_input* in, int prn, const gpsacq_peak* peak,
                                      uint64_t block_first_sample, const gpsacq_track_params* params, gpsacq_track_chan* ch) {
    if (!e || !in) return fail(GPSACQ_ERR_ARG, "gpsacq_track_start_iq8: null argument");
    Capture cap;
    if (int rc = iq8_capture(e, in, nullptr, 0, &cap)) return rc;
    gpsacq_track_params p;  // the 1-bit defaults stand in where only fll_epochs is read
    if (params) p = *params;
    else if (int rc = gpsacq_track_default_params(e, &p)) return rc;
    if (int rc = gpsacq_track_start(e, prn, peak, block_first_sample, &p, ch)) return rc;
    if (in->multibit == GPSACQ_SAMPLES_SIGN) return GPSACQ_OK;
    // the carrier in the raw capture: the search saw it turned by +mix_hz and (unless complex baseband) through Sample()'s LO at fc
    gpsacq_handoff_t h;
    if (int rc = gpsacq_handoff_engine(e, peak, 0.0, &h)) return rc;
    const double f = h.lo_dop_hz - in->mix_hz + (in->multibit == GPSACQ_SAMPLES_COMPLEX ? 0.0 : e->p.fc);
    if (!(std::fabs(f) < e->p.fs / 2)) return fail(GPSACQ_ERR_ARG, "gpsacq_track_start_iq8: carrier %g Hz outside +-fs / 2 = %g", f, e->p.fs / 2);
    const uint32_t word = (uint32_t)(int64_t)std::llround(f / e->p.fs * 4294967296.0);
    ch->lo_rate = word;
    ch->lo_int = ch->lo_nom = (int64_t)((uint64_t)word << 32);
    ch->lo_phase = (uint32_t)(ch->next_sample * (uint64_t)word);
    return GPSACQ_OK;
}

extern "C" int gpsacq_track_nominal_word_iq8(const gpsacq_engine* e, const gpsacq_iq8_input* in, uint32_t* word) {
    if (!e || !in || !word) return fail(GPSACQ_ERR_ARG, "gpsacq_track_nominal_word_iq8: null argument");
    Capture cap;
    if (int rc = iq8_capture(e, in, nullptr, 0, &cap)) return rc;
    if (in->multibit == GPSACQ_SAMPLES_SIGN) {  // gpsacq_track_start's lo_nom >> 32; cycles per sample mod 1, so that the cast is defined at fc >= fs
        const double cycles = e->p.fc / e->p.fs;
        *word = (uint32_t)((cycles - std::floor(cycles)) * 4294967296.0);
        return GPSACQ_OK;
    }
    // gpsacq_track_start_iq8's carrier at zero Doppler, folded into [-fs / 2, fs / 2)
    double f = -in->mix_hz + (in->multibit == GPSACQ_SAMPLES_COMPLEX ? 0.0 : e->p.fc);
    f -= e->p.fs * std::floor(f / e->p.fs + 0.5);
    *word = (uint32_t)(int64_t)std::llround(f / e->p.fs * 4294967296.0);
    return GPSACQ_OK;
}

extern "C" int gpsacq_track_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, uint64_t first_sample,
                                       gpsacq_track_chan* chans, int n_chans, const gpsacq_track_params* params, void* d_prompt,
                                       void* d_records, int max_epochs, int32_t* n_epochs_out) {
    if (!e || !d_iq || n_samples == 0 || !chans || n_chans <= 0 || max_epochs < 0 || !n_epochs_out)
        return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: bad argument");
    Capture cap;
    if (int rc = iq8_capture(e, in, d_iq, 0, &cap)) return rc;
    if ((uintptr_t)d_iq & 15) return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: IQ buffer must be 16-byte aligned");
    const bool sign = in->multibit == GPSACQ_SAMPLES_SIGN;
    if (sign && (first_sample & 7))
        return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: first_sample %llu is not a multiple of 8 (sign mode runs on the 1-bit stream's byte grid)",
                    (unsigned long long)first_sample);
    gpsacq_track_params p;
    if (params) p = *params;
    else if (!sign) return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: multi-bit channels need params (gpsacq_track_default_params_iq8)");
    else if (int rc = gpsacq_track_default_params(e, &p)) return rc;
    if (int rc = track_check_params(p)) return rc;
    if (int rc = track_prepare(e, first_sample, chans, n_chans)) return rc;
    if (int rc = e->tiq_t.begin(e->stream)) return rc;
    if (sign) {
        // the window as the 1-bit stream the scripts would have written, in engine scratch; then the 1-bit channels on it
        const size_t n_bytes = (n_samples + 7) / 8;
        if (int rc = e->d_iqbits.grow(n_bytes, e->stream)) return rc;
        const size_t left = cap.iq_total > cap.iq_first ? cap.iq_total - cap.iq_first : 0;  // samples of the capture from iq[0] on
        if (left < n_samples) HIPCHK(hipMemsetAsync(e->d_iqbits, 0, n_bytes, e->stream));
        if (int rc = iq8_to_bits_enqueue(e, (const uint8_t*)d_iq, std::min(n_samples, left), cap.iq, cap.iq_first, e->d_iqbits)) return rc;
        if (int rc = e->tiq_t.mark(1, e->stream)) return rc;
        track_launch_bits(e, e->d_iqbits, n_bytes, first_sample, n_chans, p, d_prompt, d_records, max_epochs);
    } else {
        if (int rc = e->tiq_t.mark(1, e->stream)) return rc;
        TrackIqArgs a{};
        track_common(e, first_sample, n_samples, n_chans, p, d_prompt, d_records, max_epochs, a);
        a.iq = (const uint8_t*)d_iq;
        a.flip = in->format == GPSACQ_IQ_U8 ? 0x80808080u : 0u;
        a.dc_i = in->remove_dc ? (int32_t)std::nearbyint(in->mean_i) : 0;
        a.dc_q = in->remove_dc ? (int32_t)std::nearbyint(in->mean_q) : 0;
        if (std::abs(a.dc_i) > 128 || std::abs(a.dc_q) > 128) return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: mean (%g, %g) outside +-128", in->mean_i, in->mean_q);
        launch_track_iq(a, e->stream);
    }
    if (int rc = e->tiq_t.mark(2, e->stream)) return rc;
    if (int rc = track_collect(e, chans, n_chans, n_epochs_out)) return rc;
    return e->tiq_t.finish();
}

extern "C" int gpsacq_track_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, uint64_t first_sample,
                                gpsacq_track_chan* chans, int n_chans, const gpsacq_track_params* params, int32_t* prompt,
                                gpsacq_track_record* records, int max_epochs, int32_t* n_epochs_out) {
    if (!e || !iq || n_samples == 0 || !chans || n_chans <= 0 || max_epochs < 0 || !n_epochs_out)
        return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_iq.grow(2 * n_samples + 16, e->stream)) return rc;
    HIPCHK(hipMemcpyAsync(e->d_iq, iq, 2 * n_samples, hipMemcpyHostToDevice, e->stream));
    return track_from_host(e, n_chans, max_epochs, prompt, records, n_epochs_out, [&](void* d_prompt, void* d_records) {
        return gpsacq_track_iq8_device(e, in, e->d_iq, n_samples, first_sample, chans, n_chans, params, d_prompt, d_records, max_epochs, n_epochs_out);
    });
}

extern "C" int gpsacq_track_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* track_ms) {
    if (!e || !e->tiq_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_track_iq8_last_ms: no finished gpsacq_track_iq8 call");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->tiq_t.elapsed(0, 1, convert_ms)) return rc;  // (the call itself waited for the stream)
    return e->tiq_t.elapsed(1, 2, track_ms);
}

// ---- NAV decoder ---------------------------------------------------------------------------------------------------------------
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
