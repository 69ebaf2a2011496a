// gpsacq_nav.cpp -- host side of "Navigation solver" of include/gpsacq.h.  First the ephemeris, host only: the fields of
// subframes 1-3 by IS-GPS-200 Tables 20-I and 20-III, read from gpsacq_subframe.words[].  Then the gpsacq_sat_states* and
// gpsacq_fix_batch* entry points that run nav_kernels.hip on the engine of gpsacq_engine.hpp.  Last "Observables": the time tag
// (host only) and the gpsacq_observables* / gpsacq_fix_track_device entry points that run obs_kernels.hip, then "Carrier observables"
// and "Velocity and clock drift": gpsacq_rate_observables*, gpsacq_sat_rates*, gpsacq_vel_batch*, gpsacq_pvt_track_device.  At the
// end "Atmosphere, elevation mask and DOP": page 18 and the parameters (host only), gpsacq_sat_views*, gpsacq_fix_atm_batch*, and
// "Fix integrity": the chi-square thresholds (host only) and gpsacq_fix_raim_batch*, which run fix_kernels.hip's k_raim_*.
// Between the velocity and the atmosphere: "Carrier-smoothed observables", gpsacq_smooth_observables* and
// gpsacq_fix_smooth_track_device, which run smooth_kernels.hip after k_code_pos and k_carrier_acc.  Then "Coarse-time
// fixes": gpsacq_coarse_obs*, gpsacq_coarse_fix_batch* and gpsacq_coarse_fix_peaks_device, which run coarse_kernels.hip, and
// "Coarse-time fix integrity": gpsacq_coarse_raim_batch*, which run its k_coarse_fix and k_coarse_exclude.  Last of
// all "Fine code phases": gpsacq_refine*, gpsacq_coarse_obs_fine* and gpsacq_coarse_fix_fine_device, which run refine_kernels.hip, and
// "Snapshot signal quality": gpsacq_snap_quality* and gpsacq_coarse_fix_quality_device, which run snapq_kernels.hip, and
// "Cold snapshot fixes": gpsacq_fine_doppler*, gpsacq_rate_obs_fine*, gpsacq_doppler_fix_batch* and gpsacq_cold_fix_device, which run
// doppler_kernels.hip, and "Snapshot chain on an 8-bit IQ capture": gpsacq_refine_iq8*, gpsacq_fine_doppler_iq8* and the two *_iq8_device
// chains, which run snapshot_iq_kernels.hip (sign mode: the conversion, then the 1-bit kernels), and "Aided acquisition": gpsacq_aid_predict*, gpsacq_aided_search* and gpsacq_aided_peaks_device, which run
// aided_kernels.hip, and "Aided acquisition on an 8-bit IQ capture": gpsacq_aided_search_iq8* and gpsacq_aided_peaks_iq8_device, which
// run aided_iq_kernels.hip (sign mode: the conversion, then k_aided), and "Coherent aided acquisition on an 8-bit IQ capture":
// gpsacq_aided_coh_search_iq8* and gpsacq_aided_coh_peaks_iq8_device, which run aided_coh_iq_kernels.hip (sign mode: the conversion,
// then k_aided_coh), and "Snapshot signal quality on an 8-bit IQ capture": gpsacq_snap_floor_iq8*, gpsacq_snap_quality_iq8* and
// gpsacq_coarse_fix_quality_iq8_device, which run snapq_iq_kernels.hip (sign mode: k_snap_quality).
// Compiled with -ffp-contract=off: the scaled fields are host floating point that tests pin bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "gpsacq_engine.hpp"
#include "atm_launch.hpp"
#include "coarse_launch.hpp"
#include "doppler_launch.hpp"
#include "nav_launch.hpp"
#include "obs_launch.hpp"
#include "raim_launch.hpp"
#include "refine_launch.hpp"
#include "aided_coh_iq_launch.hpp"
#include "aided_iq_launch.hpp"
#include "aided_launch.hpp"
#include "smooth_launch.hpp"
#include "snapq_iq_launch.hpp"
#include "snapq_launch.hpp"
#include "snapshot_iq_launch.hpp"

using namespace acq;

// ---- the shapes the entry points below are made of --------------------------------------------------------------------------
// n elements of a host array into a buffer of the engine, grown to hold them, on the engine's stream
template <class T> static int upload(gpsacq_engine* e, Scratch<T>& d, const T* src, size_t n) {
    if (int rc = d.grow(n, e->stream)) return rc;
    HIPCHK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
    return GPSACQ_OK;
}
// ... and back, where the caller wants them (dst may be NULL); the caller waits for the stream after its last one
template <class T> static int download(gpsacq_engine* e, T* dst, const Scratch<T>& d, size_t n) {
    if (dst) HIPCHK(hipMemcpyAsync(dst, d, n * sizeof(T), hipMemcpyDeviceToHost, e->stream));
    return GPSACQ_OK;
}
// an optional output of a chain: the caller's buffer, or the engine's grown to n elements
template <class T> static int or_own(gpsacq_engine* e, void*& d, Scratch<T>& own, size_t n) {
    if (d) return GPSACQ_OK;
    if (int rc = own.grow(n, e->stream)) return rc;
    d = own.p;
    return GPSACQ_OK;
}
// a one-kernel stage: the timer's two events around whatever `launch` enqueues on the stream
template <class Launch> static int timed_stage(Stages<2>& t, hipStream_t stream, Launch launch) {
    if (int rc = t.begin(stream)) return rc;
    launch();
    if (int rc = t.mark(1, stream)) return rc;
    return t.finish();
}
// the time of a one-kernel stage: waited for where it ran, exactly 0 where it did not
static int stage_ms(const Stages<2>& t, float* ms) {
    float v = 0.f;
    if (t.ran()) {
        if (int rc = t.wait()) return rc;
        if (int rc = t.elapsed(0, 1, &v)) return rc;
    }
    if (ms) *ms = v;
    return GPSACQ_OK;
}
// the records of a host-buffer form into e->d_obs_rec: the rows keep their stride; only the records that exist travel
static int upload_records(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs, int n_chans) {
    if (int rc = e->d_obs_rec.grow((size_t)n_chans * (size_t)std::max(max_epochs, 1), e->stream)) return rc;
    for (int c = 0; c < n_chans; ++c)
        if (n_epochs[c] > 0)
            HIPCHK(hipMemcpyAsync(e->d_obs_rec + (size_t)c * max_epochs, records + (size_t)c * max_epochs,
                                  (size_t)n_epochs[c] * sizeof(gpsacq_track_record), hipMemcpyHostToDevice, e->stream));
    return GPSACQ_OK;
}

// ---- ephemeris ---------------------------------------------------------------------------------------------------------------
namespace {
constexpr double GPS_PI = 3.1415926535898;

// n bits (<= 32) that start at bit `bit` (1..24) of ICD word `word` (1..10) and run on into the data bits of the next word
uint32_t ubits(const uint32_t* words, int word, int bit, int n) {
    uint32_t v = 0;
    int pos = (word - 1) * 24 + (bit - 1);  // index into the 240 data bits d1..d24 of the ten words
    for (int k = 0; k < n; ++k, ++pos) v = (v << 1) | ((words[pos / 24] >> (23 - pos % 24)) & 1u);
    return v;
}
int32_t sbits(const uint32_t* words, int word, int bit, int n) {
    const uint32_t v = ubits(words, word, bit, n);
    return n < 32 && (v >> (n - 1)) ? (int32_t)v - (int32_t)(1u << n) : (int32_t)v;
}
double scaled(double field, int exp2) { return std::ldexp(field, exp2); }
double semicircles(double field, int exp2) { return std::ldexp(field, exp2) * GPS_PI; }
}  // namespace

extern "C" int gpsacq_ephemeris_load(gpsacq_ephemeris* eph, const gpsacq_subframe* sf, int n) {
    if (!eph || n < 0 || (n > 0 && !sf)) return fail(GPSACQ_ERR_ARG, "gpsacq_ephemeris_load: bad argument");
    for (int k = 0; k < n; ++k) {
        const uint32_t* w = sf[k].words;
        const int id = (int)ubits(w, 2, 20, 3);
        if (id < 1 || id > 3) continue;
        eph->tow = (int32_t)ubits(w, 2, 1, 17);
        eph->have |= 1 << (id - 1);
        if (id == 1) {  // Table 20-I
            eph->week = ubits(w, 3, 1, 10);
            eph->iodc = ubits(w, 3, 23, 2) << 8 | ubits(w, 8, 1, 8);
            eph->t_gd = scaled(sbits(w, 7, 17, 8), -31);
            eph->t_oc = ubits(w, 8, 9, 16) * 16u;
            eph->a_f2 = scaled(sbits(w, 9, 1, 8), -55);
            eph->a_f1 = scaled(sbits(w, 9, 9, 16), -43);
            eph->a_f0 = scaled(sbits(w, 10, 1, 22), -31);
        } else if (id == 2) {  // Table 20-III, subframe 2
            eph->iode2 = ubits(w, 3, 1, 8);
            eph->c_rs = scaled(sbits(w, 3, 9, 16), -5);
            eph->dn = semicircles(sbits(w, 4, 1, 16), -43);
            eph->m_0 = semicircles(sbits(w, 4, 17, 32), -31);
            eph->c_uc = scaled(sbits(w, 6, 1, 16), -29);
            eph->e = scaled(ubits(w, 6, 17, 32), -33);
            eph->c_us = scaled(sbits(w, 8, 1, 16), -29);
            eph->sqrt_a = scaled(ubits(w, 8, 17, 32), -19);
            eph->t_oe = ubits(w, 10, 1, 16) * 16u;
        } else {  // subframe 3
            eph->c_ic = scaled(sbits(w, 3, 1, 16), -29);
            eph->omega_0 = semicircles(sbits(w, 3, 17, 32), -31);
            eph->c_is = scaled(sbits(w, 5, 1, 16), -29);
            eph->i_0 = semicircles(sbits(w, 5, 17, 32), -31);
            eph->c_rc = scaled(sbits(w, 7, 1, 16), -5);
            eph->omega = semicircles(sbits(w, 7, 17, 32), -31);
            eph->omega_dot = semicircles(sbits(w, 9, 1, 24), -43);
            eph->iode3 = ubits(w, 10, 1, 8);
            eph->idot = semicircles(sbits(w, 10, 9, 14), -43);
        }
    }
    return GPSACQ_OK;
}

extern "C" int gpsacq_ephemeris_valid(const gpsacq_ephemeris* eph) {
    if (!eph || (eph->have & 7) != 7) return 0;
    return eph->iode2 != 0 && (eph->iodc & 0xffu) == eph->iode2 && eph->iode2 == eph->iode3;
}

// ---- satellite state and fixes (nav_kernels.hip) ----------------------------------------------------------------------------
// the call's ephemerides as the kernels read them, into e->d_nav_eph
static int nav_upload_eph(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph) {
    std::vector<NavEph> tab((size_t)n_eph);
    for (int k = 0; k < n_eph; ++k) {
        const gpsacq_ephemeris& s = eph[k];
        NavEph& d = tab[k];
        d.t_gd = s.t_gd, d.a_f0 = s.a_f0, d.a_f1 = s.a_f1, d.a_f2 = s.a_f2;
        d.c_rs = s.c_rs, d.dn = s.dn, d.m_0 = s.m_0, d.c_uc = s.c_uc, d.e = s.e, d.c_us = s.c_us, d.sqrt_a = s.sqrt_a;
        d.c_ic = s.c_ic, d.omega_0 = s.omega_0, d.c_is = s.c_is, d.i_0 = s.i_0, d.c_rc = s.c_rc, d.omega = s.omega;
        d.omega_dot = s.omega_dot, d.idot = s.idot;
        // t_oc, t_oe: 16-bit fields * 16 s <= 1 048 560 s, so the milliseconds fit an int32; an epoch past the week is not an ephemeris
        const bool in_week = s.t_oc < 604800u && s.t_oe < 604800u;
        d.toc_ms = in_week ? (int32_t)(s.t_oc * 1000u) : 0;
        d.toe_ms = in_week ? (int32_t)(s.t_oe * 1000u) : 0;
        d.valid = in_week && gpsacq_ephemeris_valid(&s);
        d.reserved = 0;
    }
    return upload(e, e->d_nav_eph, tab.data(), tab.size());  // pageable source: the copy has left `tab` when the call returns
}

static int nav_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, size_t n, const void* out) {
    if (!e || !eph || n_eph <= 0 || !obs || !out || n == 0 || n > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    return GPSACQ_OK;
}
static int nav_check_weights(const char* who, const gpsacq_obs* obs, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!(obs[k].weight >= 0.0) || !std::isfinite(obs[k].weight))
            return fail(GPSACQ_ERR_ARG, "%s: observation %zu has weight %g (must be finite and >= 0)", who, k, obs[k].weight);
    return GPSACQ_OK;
}

extern "C" int gpsacq_sat_states_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_obs,
                                        void* d_out, int sync) {
    if (int rc = nav_check("gpsacq_sat_states", e, eph, n_eph, d_obs, n_obs, d_out)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, (gpsacq_sat_state*)d_out}, e->stream);
    HIPCHK(hipGetLastError());
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_sat_states(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_obs,
                                 gpsacq_sat_state* out) {
    if (int rc = nav_check("gpsacq_sat_states", e, eph, n_eph, obs, n_obs, out)) return rc;
    if (int rc = nav_check_weights("gpsacq_sat_states", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = gpsacq_sat_states_device(e, eph, n_eph, e->d_nav_obs, n_obs, e->d_nav_state, 0)) return rc;
    if (int rc = download(e, out, e->d_nav_state, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                       int sats_per_fix, void* d_out, int sync) {
    if (int rc = nav_check("gpsacq_fix_batch", e, eph, n_eph, d_obs, n_fix, d_out)) return rc;
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "gpsacq_fix_batch: sats_per_fix %d outside 1 .. %d", sats_per_fix, GPSACQ_FIX_MAX_SATS);
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    if (int rc = e->nav_t.begin(e->stream)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_nav_state}, e->stream);
    if (int rc = e->nav_t.mark(1, e->stream)) return rc;
    launch_fix(FixArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, e->d_nav_state, n_fix, sats_per_fix, (gpsacq_fix*)d_out}, e->stream);
    if (int rc = e->nav_t.mark(2, e->stream)) return rc;
    if (int rc = e->nav_t.finish()) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_fix,
                                int sats_per_fix, gpsacq_fix* out) {
    if (int rc = nav_check("gpsacq_fix_batch", e, eph, n_eph, obs, n_fix, out)) return rc;
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "gpsacq_fix_batch: sats_per_fix %d outside 1 .. %d", sats_per_fix, GPSACQ_FIX_MAX_SATS);
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_fix_batch", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_nav_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = gpsacq_fix_batch_device(e, eph, n_eph, e->d_nav_obs, n_fix, sats_per_fix, e->d_nav_fix, 0)) return rc;
    if (int rc = download(e, out, e->d_nav_fix, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* fix_ms) {
    if (!e || !e->nav_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_last_ms: no gpsacq_fix_batch call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->nav_t.wait()) return rc;
    if (int rc = e->nav_t.elapsed(0, 1, sat_state_ms)) return rc;
    return e->nav_t.elapsed(1, 2, fix_ms);
}

// ---- observables (obs_kernels.hip) ------------------------------------------------------------------------------------------
extern "C" int gpsacq_time_tag_from_subframe(const gpsacq_subframe* sf, int bit_epoch0, int eph_index, gpsacq_time_tag* tag) {
    if (!sf || !tag) return fail(GPSACQ_ERR_ARG, "gpsacq_time_tag_from_subframe: null argument");
    if (sf->tow < 0 || sf->tow > 100799) return fail(GPSACQ_ERR_ARG, "gpsacq_time_tag_from_subframe: TOW count %d outside 0 .. 100799", sf->tow);
    tag->epoch = bit_epoch0 + 20 * sf->bit_offset;
    tag->ms = (sf->tow + 100799) % 100800 * 6000;  // the count names the start of the NEXT subframe
    tag->eph = eph_index;
    tag->valid = 1;
    return GPSACQ_OK;
}

// what the code and the carrier observables share: the records of one tracking call and the receive instants
static int records_check(const char* who, const gpsacq_engine* e, const void* records, int max_epochs, const int32_t* n_epochs,
                         const gpsacq_track_chan* chans, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix) {
    if (!e || !records || !n_epochs || !chans || max_epochs < 0 || n_fix == 0 || n_fix > ((size_t)1 << 31))
        return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (n_chans < 1 || n_chans > GPSACQ_FIX_MAX_SATS) return fail(GPSACQ_ERR_ARG, "%s: n_chans %d outside 1 .. %d", who, n_chans, GPSACQ_FIX_MAX_SATS);
    if (rx_step == 0) return fail(GPSACQ_ERR_ARG, "%s: rx_step must be at least 1", who);
    if ((uint64_t)(n_fix - 1) > (UINT64_MAX - first_rx_sample) / rx_step)
        return fail(GPSACQ_ERR_ARG, "%s: the last receive instant does not fit 64 bits", who);
    for (int c = 0; c < n_chans; ++c)
        if (n_epochs[c] < 0 || n_epochs[c] > max_epochs)
            return fail(GPSACQ_ERR_ARG, "%s: channel %d has %d epochs, max_epochs is %d", who, c, n_epochs[c], max_epochs);
    return GPSACQ_OK;
}

static int obs_check(const char* who, const gpsacq_engine* e, const void* records, int max_epochs, const int32_t* n_epochs,
                     const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample, uint64_t rx_step,
                     size_t n_fix) {
    if (!tags) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    return records_check(who, e, records, max_epochs, n_epochs, chans, n_chans, first_rx_sample, rx_step, n_fix);
}

// the call's channels as the kernels read them into e->d_obs_chan, then k_code_pos as the first stage of obs_t
static int code_pos_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                            const gpsacq_time_tag* tags, int n_chans) {
    ObsChan tab[GPSACQ_FIX_MAX_SATS];
    for (int c = 0; c < n_chans; ++c) {
        ObsChan& d = tab[c];
        d.ca_pos = chans[c].ca_pos, d.next_sample = chans[c].next_sample;
        d.n = n_epochs[c];
        d.first_epoch = (int32_t)((uint32_t)chans[c].epoch - (uint32_t)n_epochs[c]);
        d.tag_epoch = tags[c].epoch, d.tag_ms = tags[c].ms, d.tag_eph = tags[c].eph, d.tag_valid = tags[c].valid;
    }
    if (int rc = e->d_obs_chan.grow((size_t)GPSACQ_FIX_MAX_SATS, e->stream)) return rc;
    if (int rc = e->d_obs_pos.grow((size_t)n_chans * (size_t)std::max(max_epochs, 1), e->stream)) return rc;
    // pageable source: the copy has left `tab` when the call returns
    HIPCHK(hipMemcpyAsync(e->d_obs_chan, tab, (size_t)n_chans * sizeof(ObsChan), hipMemcpyHostToDevice, e->stream));
    if (int rc = e->obs_t.begin(e->stream)) return rc;
    launch_code_pos(CodePosArgs{e->d_obs_chan, (const gpsacq_track_record*)d_records, max_epochs, e->d_obs_pos}, n_chans, e->stream);
    if (int rc = e->obs_t.mark(1, e->stream)) return rc;
    return GPSACQ_OK;
}

// both kernels on the engine's stream; every argument has been checked
static int obs_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                       const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, void* d_obs) {
    if (int rc = code_pos_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans)) return rc;
    launch_observe(ObserveArgs{e->d_obs_chan, (const gpsacq_track_record*)d_records, e->d_obs_pos, max_epochs, n_chans, first_rx_sample, rx_step,
                               n_fix, (gpsacq_obs*)d_obs},
                   e->stream);
    if (int rc = e->obs_t.mark(2, e->stream)) return rc;
    if (int rc = e->obs_t.finish()) return rc;
    return GPSACQ_OK;
}

extern "C" int gpsacq_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                         const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                         uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, void* d_obs, int sync) {
    if (int rc = obs_check("gpsacq_observables", e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    if (!d_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = obs_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, d_obs)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                  const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                  uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, gpsacq_obs* obs) {
    if (int rc = obs_check("gpsacq_observables", e, records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    if (!obs) return fail(GPSACQ_ERR_ARG, "gpsacq_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_nav_obs.grow(n_obs, e->stream)) return rc;
    if (int rc = upload_records(e, records, max_epochs, n_epochs, n_chans)) return rc;
    if (int rc = obs_enqueue(e, e->d_obs_rec, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, e->d_nav_obs)) return rc;
    if (int rc = download(e, obs, e->d_nav_obs, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                       const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                       uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, void* d_obs, void* d_fix, int sync) {
    if (int rc = obs_check("gpsacq_fix_track", e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_fix) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_track: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_obs, e->d_nav_obs, n_fix * (size_t)n_chans)) return rc;
    if (int rc = obs_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, d_obs)) return rc;
    return gpsacq_fix_batch_device(e, eph, n_eph, d_obs, n_fix, n_chans, d_fix, sync);
}

extern "C" int gpsacq_observables_last_ms(const gpsacq_engine* e, float* code_pos_ms, float* observe_ms) {
    if (!e || !e->obs_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_observables_last_ms: no gpsacq_observables call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->obs_t.wait()) return rc;
    if (int rc = e->obs_t.elapsed(0, 1, code_pos_ms)) return rc;
    return e->obs_t.elapsed(1, 2, observe_ms);
}

// ---- carrier observables (obs_kernels.hip) ---------------------------------------------------------------------------------
static int rate_check(const char* who, const gpsacq_engine* e, const void* records, int max_epochs, const int32_t* n_epochs,
                      const gpsacq_track_chan* chans, const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step,
                      size_t n_fix, uint64_t avg_samples) {
    if (!nom_words) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = records_check(who, e, records, max_epochs, n_epochs, chans, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    if (avg_samples == 0) return fail(GPSACQ_ERR_ARG, "%s: avg_samples must be at least 1", who);
    return GPSACQ_OK;
}

// the call's channels as the carrier kernels read them into e->d_rate_chan, then k_carrier_acc as the first stage of rate_t
static int carrier_acc_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                               const uint32_t* nom_words, int n_chans) {
    RateChan tab[GPSACQ_FIX_MAX_SATS];
    for (int c = 0; c < n_chans; ++c) tab[c] = RateChan{chans[c].next_sample, n_epochs[c], nom_words[c]};
    if (int rc = e->d_rate_chan.grow((size_t)GPSACQ_FIX_MAX_SATS, e->stream)) return rc;
    if (int rc = e->d_rate_acc.grow((size_t)n_chans * ((size_t)max_epochs + 1), e->stream)) return rc;
    // pageable source: the copy has left `tab` when the call returns
    HIPCHK(hipMemcpyAsync(e->d_rate_chan, tab, (size_t)n_chans * sizeof(RateChan), hipMemcpyHostToDevice, e->stream));
    if (int rc = e->rate_t.begin(e->stream)) return rc;
    launch_carrier_acc(CarrierAccArgs{e->d_rate_chan, (const gpsacq_track_record*)d_records, max_epochs, e->d_rate_acc}, n_chans, e->stream);
    if (int rc = e->rate_t.mark(1, e->stream)) return rc;
    return GPSACQ_OK;
}

// both kernels on the engine's stream; every argument has been checked
static int rate_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                        const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, uint64_t avg_samples,
                        void* d_rate_obs) {
    if (int rc = carrier_acc_enqueue(e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans)) return rc;
    launch_observe_rate(ObserveRateArgs{e->d_rate_chan, (const gpsacq_track_record*)d_records, e->d_rate_acc, max_epochs, n_chans, first_rx_sample,
                                        rx_step, avg_samples, e->p.fs, n_fix, (gpsacq_rate_obs*)d_rate_obs},
                        e->stream);
    if (int rc = e->rate_t.mark(2, e->stream)) return rc;
    if (int rc = e->rate_t.finish()) return rc;
    return GPSACQ_OK;
}

extern "C" int gpsacq_rate_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                              const gpsacq_track_chan* chans, const uint32_t* nom_words, int n_chans,
                                              uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, uint64_t avg_samples,
                                              void* d_rate_obs, int sync) {
    if (int rc = rate_check("gpsacq_rate_observables", e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples)) return rc;
    if (!d_rate_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_rate_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = rate_enqueue(e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples, d_rate_obs)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_rate_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                       const gpsacq_track_chan* chans, const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample,
                                       uint64_t rx_step, size_t n_fix, uint64_t avg_samples, gpsacq_rate_obs* rate_obs) {
    if (int rc = rate_check("gpsacq_rate_observables", e, records, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples)) return rc;
    if (!rate_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_rate_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_rate_obs.grow(n_obs, e->stream)) return rc;
    if (int rc = upload_records(e, records, max_epochs, n_epochs, n_chans)) return rc;
    if (int rc = rate_enqueue(e, e->d_obs_rec, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples, e->d_rate_obs)) return rc;
    if (int rc = download(e, rate_obs, e->d_rate_obs, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

// ---- velocity and clock drift (nav_kernels.hip) ----------------------------------------------------------------------------
extern "C" int gpsacq_sat_rates_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_obs,
                                       void* d_out, int sync) {
    if (int rc = nav_check("gpsacq_sat_rates", e, eph, n_eph, d_obs, n_obs, d_out)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    launch_sat_state_rate(SatRateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, (gpsacq_sat_rate*)d_out}, e->stream);
    HIPCHK(hipGetLastError());
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_sat_rates(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_obs,
                                gpsacq_sat_rate* out) {
    if (int rc = nav_check("gpsacq_sat_rates", e, eph, n_eph, obs, n_obs, out)) return rc;
    if (int rc = nav_check_weights("gpsacq_sat_rates", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_sat_rate.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = gpsacq_sat_rates_device(e, eph, n_eph, e->d_nav_obs, n_obs, e->d_sat_rate, 0)) return rc;
    if (int rc = download(e, out, e->d_sat_rate, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

static int vel_check(const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, const void* rate_obs, const void* fixes,
                     size_t n_fix, int sats_per_fix, const void* out) {
    if (int rc = nav_check("gpsacq_vel_batch", e, eph, n_eph, obs, n_fix, out)) return rc;
    if (!rate_obs || !fixes) return fail(GPSACQ_ERR_ARG, "gpsacq_vel_batch: bad argument");
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "gpsacq_vel_batch: sats_per_fix %d outside 1 .. %d", sats_per_fix, GPSACQ_FIX_MAX_SATS);
    return GPSACQ_OK;
}

// k_sat_state_rate and k_vel on the engine's stream; e->d_nav_eph holds the call's ephemerides and e->d_nav_state the satellite
// states of d_obs (enqueued before), every argument has been checked
static int vel_enqueue(gpsacq_engine* e, int n_eph, const void* d_obs, const void* d_rate_obs, const void* d_fixes, size_t n_fix,
                       int sats_per_fix, void* d_out) {
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = e->d_sat_rate.grow(n_obs, e->stream)) return rc;
    if (int rc = e->vel_t.begin(e->stream)) return rc;
    launch_sat_state_rate(SatRateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_sat_rate}, e->stream);
    if (int rc = e->vel_t.mark(1, e->stream)) return rc;
    launch_vel(VelArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, (const gpsacq_rate_obs*)d_rate_obs, e->d_nav_state, e->d_sat_rate,
                       (const gpsacq_fix*)d_fixes, n_fix, sats_per_fix, (gpsacq_vel*)d_out},
               e->stream);
    if (int rc = e->vel_t.mark(2, e->stream)) return rc;
    if (int rc = e->vel_t.finish()) return rc;
    return GPSACQ_OK;
}

extern "C" int gpsacq_vel_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_rate_obs,
                                       const void* d_fixes, size_t n_fix, int sats_per_fix, void* d_out, int sync) {
    if (int rc = vel_check(e, eph, n_eph, d_obs, d_rate_obs, d_fixes, n_fix, sats_per_fix, d_out)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_nav_state}, e->stream);
    if (int rc = vel_enqueue(e, n_eph, d_obs, d_rate_obs, d_fixes, n_fix, sats_per_fix, d_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_vel_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs,
                                const gpsacq_rate_obs* rate_obs, const gpsacq_fix* fixes, size_t n_fix, int sats_per_fix, gpsacq_vel* out) {
    if (int rc = vel_check(e, eph, n_eph, obs, rate_obs, fixes, n_fix, sats_per_fix, out)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_vel_batch", obs, n_obs)) return rc;
    for (size_t k = 0; k < n_obs; ++k)
        if (!(rate_obs[k].weight >= 0.0) || !std::isfinite(rate_obs[k].weight))
            return fail(GPSACQ_ERR_ARG, "gpsacq_vel_batch: rate observation %zu has weight %g (must be finite and >= 0)", k, rate_obs[k].weight);
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_vel.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_rate_obs, rate_obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_nav_fix, fixes, n_fix)) return rc;
    if (int rc = gpsacq_vel_batch_device(e, eph, n_eph, e->d_nav_obs, e->d_rate_obs, e->d_nav_fix, n_fix, sats_per_fix, e->d_vel, 0)) return rc;
    if (int rc = download(e, out, e->d_vel, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_pvt_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                       const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                       const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                       uint64_t avg_samples, void* d_obs, void* d_rate_obs, void* d_fix, void* d_vel, int sync) {
    if (int rc = rate_check("gpsacq_pvt_track", e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples)) return rc;
    if (!tags || !eph || n_eph <= 0 || !d_fix || !d_vel) return fail(GPSACQ_ERR_ARG, "gpsacq_pvt_track: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_obs, e->d_nav_obs, n_fix * (size_t)n_chans)) return rc;
    if (int rc = or_own(e, d_rate_obs, e->d_rate_obs, n_fix * (size_t)n_chans)) return rc;
    if (int rc = obs_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, d_obs)) return rc;
    if (int rc = rate_enqueue(e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans, first_rx_sample, rx_step, n_fix, avg_samples, d_rate_obs)) return rc;
    if (int rc = gpsacq_fix_batch_device(e, eph, n_eph, d_obs, n_fix, n_chans, d_fix, 0)) return rc;
    // the ephemerides and the satellite states of d_obs are on the device from the fixes: only the rates and the solve remain
    if (int rc = vel_enqueue(e, n_eph, d_obs, d_rate_obs, d_fix, n_fix, n_chans, d_vel)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_velocity_last_ms(const gpsacq_engine* e, float* carrier_acc_ms, float* observe_rate_ms, float* sat_rate_ms, float* vel_ms) {
    if (!e || (!e->rate_t.ran() && !e->vel_t.ran())) return fail(GPSACQ_ERR_ARG, "gpsacq_velocity_last_ms: no rate or velocity call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    float t[4] = {0.f, 0.f, 0.f, 0.f};  // the half that did not run reads 0
    const Stages<3>* half[2] = {&e->rate_t, &e->vel_t};
    for (int h = 0; h < 2; ++h)
        if (half[h]->ran()) {
            if (int rc = half[h]->wait()) return rc;
            if (int rc = half[h]->elapsed(0, 1, &t[2 * h])) return rc;
            if (int rc = half[h]->elapsed(1, 2, &t[2 * h + 1])) return rc;
        }
    if (carrier_acc_ms) *carrier_acc_ms = t[0];
    if (observe_rate_ms) *observe_rate_ms = t[1];
    if (sat_rate_ms) *sat_rate_ms = t[2];
    if (vel_ms) *vel_ms = t[3];
    return GPSACQ_OK;
}

// ---- carrier-smoothed observables (smooth_kernels.hip) --------------------------------------------------------------------
extern "C" int gpsacq_smooth_default_params(gpsacq_smooth_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_smooth_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->window = 1000;
    p->lock_epochs = 20;
    p->lock_num = 1, p->lock_den = 2;
    p->jump = (int64_t)385 << 32;  // a quarter chip in carrier cycles
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int smooth_params(const char* who, const gpsacq_smooth_params* params, gpsacq_smooth_params* out) {
    if (!params) return gpsacq_smooth_default_params(out);
    *out = *params;
    if (out->window < 1 || out->window > 65536) return fail(GPSACQ_ERR_ARG, "%s: window %d outside 1 .. 65536", who, out->window);
    if (out->lock_epochs < 0 || out->lock_epochs > 1024) return fail(GPSACQ_ERR_ARG, "%s: lock_epochs %d outside 0 .. 1024", who, out->lock_epochs);
    if (out->lock_num < 1 || out->lock_num > out->lock_den || out->lock_den > 1024)
        return fail(GPSACQ_ERR_ARG, "%s: lock_num / lock_den %d / %d outside 1 <= num <= den <= 1024", who, out->lock_num, out->lock_den);
    if (out->jump < 0) return fail(GPSACQ_ERR_ARG, "%s: jump must not be negative", who);
    return GPSACQ_OK;
}

static int smooth_check(const char* who, const gpsacq_engine* e, const void* records, int max_epochs, const int32_t* n_epochs,
                        const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, const uint32_t* nom_words, int n_chans,
                        uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, const gpsacq_smooth_params* params, gpsacq_smooth_params* checked) {
    if (!tags || !nom_words) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = records_check(who, e, records, max_epochs, n_epochs, chans, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    return smooth_params(who, params, checked);
}

// k_code_pos, k_carrier_acc and the four smoothing kernels on the engine's stream; every argument has been checked
static int smooth_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                          const gpsacq_time_tag* tags, const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step,
                          size_t n_fix, const gpsacq_smooth_params& sp, void* d_obs, void* d_info) {
    SmoothChan tab[GPSACQ_FIX_MAX_SATS];
    for (int c = 0; c < n_chans; ++c) {
        SmoothChan& d = tab[c];
        d.next_sample = chans[c].next_sample;
        d.n = n_epochs[c];
        d.first_epoch = (int32_t)((uint32_t)chans[c].epoch - (uint32_t)n_epochs[c]);
        d.tag_epoch = tags[c].epoch, d.tag_ms = tags[c].ms, d.tag_eph = tags[c].eph, d.tag_valid = tags[c].valid;
        d.cw = (uint32_t)((uint64_t)chans[c].ca_nom >> 32);
        d.nom_word = nom_words[c];
    }
    const size_t row = (size_t)max_epochs + 1, nc = (size_t)n_chans;
    if (int rc = e->d_smooth_chan.grow((size_t)GPSACQ_FIX_MAX_SATS, e->stream)) return rc;
    if (int rc = e->d_smooth_lock.grow(2 * nc * row, e->stream)) return rc;
    if (int rc = e->d_smooth_q.grow(nc * (3 * n_fix + 1), e->stream)) return rc;
    if (int rc = e->d_smooth_w.grow(nc * 3 * n_fix, e->stream)) return rc;
    // pageable source: the copy has left `tab` when the call returns
    HIPCHK(hipMemcpyAsync(e->d_smooth_chan, tab, nc * sizeof(SmoothChan), hipMemcpyHostToDevice, e->stream));
    // pos_t and A_t into the scratch the observables use; their second kernels do not run, so those times read 0
    if (int rc = code_pos_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans)) return rc;
    if (int rc = e->obs_t.mark(2, e->stream)) return rc;
    if (int rc = e->obs_t.finish()) return rc;
    if (int rc = carrier_acc_enqueue(e, d_records, max_epochs, n_epochs, chans, nom_words, n_chans)) return rc;
    if (int rc = e->rate_t.mark(2, e->stream)) return rc;
    if (int rc = e->rate_t.finish()) return rc;
    const gpsacq_track_record* rec = (const gpsacq_track_record*)d_records;
    int64_t *lock_n = e->d_smooth_lock, *lock_d = e->d_smooth_lock + nc * row;
    uint64_t *z = e->d_smooth_q, *p = z + nc * n_fix, *sum = p + nc * n_fix;
    int32_t *t = e->d_smooth_w, *state = t + nc * n_fix, *seg = state + nc * n_fix;
    if (int rc = e->smooth_t.begin(e->stream)) return rc;
    if (sp.lock_epochs > 0) launch_lock_acc(LockAccArgs{e->d_smooth_chan, rec, max_epochs, lock_n, lock_d}, n_chans, e->stream);
    if (int rc = e->smooth_t.mark(1, e->stream)) return rc;
    launch_cmc(CmcArgs{e->d_smooth_chan, rec, e->d_obs_pos, e->d_rate_acc, lock_n, lock_d, max_epochs, n_chans, first_rx_sample, rx_step, n_fix,
                       sp.lock_epochs, sp.lock_num, sp.lock_den, sp.invert, z, p, t, state},
               e->stream);
    if (int rc = e->smooth_t.mark(2, e->stream)) return rc;
    launch_smooth_scan(SmoothScanArgs{z, state, n_fix, sp.jump, sum, seg}, n_chans, e->stream);
    if (int rc = e->smooth_t.mark(3, e->stream)) return rc;
    launch_smooth_out(SmoothOutArgs{e->d_smooth_chan, z, p, t, state, sum, seg, n_chans, n_fix, sp.window, (gpsacq_obs*)d_obs,
                                    (gpsacq_smooth_info*)d_info},
                      e->stream);
    if (int rc = e->smooth_t.mark(4, e->stream)) return rc;
    if (int rc = e->smooth_t.finish()) return rc;
    return GPSACQ_OK;
}

extern "C" int gpsacq_smooth_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                                const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, const uint32_t* nom_words,
                                                int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                                const gpsacq_smooth_params* params, void* d_obs, void* d_info, int sync) {
    gpsacq_smooth_params sp;
    if (int rc = smooth_check("gpsacq_smooth_observables", e, d_records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, params, &sp)) return rc;
    if (!d_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_smooth_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = smooth_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, sp, d_obs, d_info)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_smooth_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                         const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, const uint32_t* nom_words, int n_chans,
                                         uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, const gpsacq_smooth_params* params,
                                         gpsacq_obs* obs, gpsacq_smooth_info* info) {
    gpsacq_smooth_params sp;
    if (int rc = smooth_check("gpsacq_smooth_observables", e, records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, params, &sp)) return rc;
    if (!obs) return fail(GPSACQ_ERR_ARG, "gpsacq_smooth_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_nav_obs.grow(n_obs, e->stream)) return rc;
    if (info)
        if (int rc = e->d_smooth_info.grow(n_obs, e->stream)) return rc;
    if (int rc = upload_records(e, records, max_epochs, n_epochs, n_chans)) return rc;
    if (int rc = smooth_enqueue(e, e->d_obs_rec, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, sp, e->d_nav_obs,
                                info ? e->d_smooth_info.p : nullptr))
        return rc;
    if (int rc = download(e, obs, e->d_nav_obs, n_obs)) return rc;
    if (int rc = download(e, info, e->d_smooth_info, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_smooth_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                              const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                              const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                              const gpsacq_smooth_params* params, void* d_obs, void* d_info, void* d_fix, int sync) {
    gpsacq_smooth_params sp;
    if (int rc = smooth_check("gpsacq_fix_smooth_track", e, d_records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, params, &sp)) return rc;
    if (!eph || n_eph <= 0 || !d_fix) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_smooth_track: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_obs, e->d_nav_obs, n_fix * (size_t)n_chans)) return rc;
    if (int rc = smooth_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, sp, d_obs, d_info)) return rc;
    return gpsacq_fix_batch_device(e, eph, n_eph, d_obs, n_fix, n_chans, d_fix, sync);
}

extern "C" int gpsacq_smooth_last_ms(const gpsacq_engine* e, float* lock_acc_ms, float* cmc_ms, float* scan_ms, float* out_ms) {
    if (!e || !e->smooth_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_smooth_last_ms: no gpsacq_smooth_observables call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->smooth_t.wait()) return rc;
    float* out[4] = {lock_acc_ms, cmc_ms, scan_ms, out_ms};
    for (int k = 0; k < 4; ++k)
        if (int rc = e->smooth_t.elapsed(k, k + 1, out[k])) return rc;
    return GPSACQ_OK;
}

// ---- signal quality per observation (quality_kernels.hip) -----------------------------------------------------------------
extern "C" int gpsacq_quality_default_params(gpsacq_quality_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_quality_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->epochs = 200;
    p->min_epochs = 20;
    p->lock_num = 1, p->lock_den = 2;
    p->require_lock = 1;
    p->cn0_min_lin = std::pow(10.0, 30.0 / 10.0);
    p->cn0_ref_lin = std::pow(10.0, 45.0 / 10.0);
    p->cn0_cap_dbhz = 99.0;
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int quality_params(const char* who, const gpsacq_quality_params* params, gpsacq_quality_params* out) {
    if (!params) return gpsacq_quality_default_params(out);
    *out = *params;
    if (out->min_epochs < 1 || out->min_epochs > out->epochs || out->epochs > 1024)
        return fail(GPSACQ_ERR_ARG, "%s: min_epochs / epochs %d / %d outside 1 <= min_epochs <= epochs <= 1024", who, out->min_epochs, out->epochs);
    if (out->lock_num < 1 || out->lock_num > out->lock_den || out->lock_den > 1024)
        return fail(GPSACQ_ERR_ARG, "%s: lock_num / lock_den %d / %d outside 1 <= num <= den <= 1024", who, out->lock_num, out->lock_den);
    if (!(out->cn0_min_lin >= 0.0) || !std::isfinite(out->cn0_min_lin)) return fail(GPSACQ_ERR_ARG, "%s: cn0_min_lin %g must be finite and >= 0", who, out->cn0_min_lin);
    if (!(out->cn0_ref_lin > 0.0) || !std::isfinite(out->cn0_ref_lin)) return fail(GPSACQ_ERR_ARG, "%s: cn0_ref_lin %g must be finite and > 0", who, out->cn0_ref_lin);
    if (!std::isfinite(out->cn0_cap_dbhz)) return fail(GPSACQ_ERR_ARG, "%s: cn0_cap_dbhz must be finite", who);
    return GPSACQ_OK;
}

static int quality_check(const char* who, const gpsacq_engine* e, const void* records, int max_epochs, const int32_t* n_epochs,
                         const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample, uint64_t rx_step,
                         size_t n_fix, const gpsacq_quality_params* params, gpsacq_quality_params* checked) {
    if (int rc = obs_check(who, e, records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix)) return rc;
    return quality_params(who, params, checked);
}

// both kernels on the engine's stream, into scratch of their own; every argument has been checked
static int quality_enqueue(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs, const gpsacq_track_chan* chans,
                           const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                           const gpsacq_quality_params& qp, void* d_obs, void* d_info) {
    QualityChan tab[GPSACQ_FIX_MAX_SATS];
    for (int c = 0; c < n_chans; ++c) {
        tab[c].next_sample = chans[c].next_sample;
        tab[c].n = n_epochs[c];
        tab[c].tag_valid = tags[c].valid;
    }
    const size_t row = (size_t)max_epochs + 1, nc = (size_t)n_chans;
    if (int rc = e->d_quality_chan.grow((size_t)GPSACQ_FIX_MAX_SATS, e->stream)) return rc;
    if (int rc = e->d_quality_sums.grow(3 * nc * row, e->stream)) return rc;
    // pageable source: the copy has left `tab` when the call returns
    HIPCHK(hipMemcpyAsync(e->d_quality_chan, tab, nc * sizeof(QualityChan), hipMemcpyHostToDevice, e->stream));
    const gpsacq_track_record* rec = (const gpsacq_track_record*)d_records;
    uint64_t *sum_a = e->d_quality_sums, *sum_d = sum_a + nc * row, *sum_n = sum_d + nc * row;
    if (int rc = e->quality_t.begin(e->stream)) return rc;
    launch_quality_acc(QualityAccArgs{e->d_quality_chan, rec, max_epochs, sum_a, sum_d, sum_n}, n_chans, e->stream);
    if (int rc = e->quality_t.mark(1, e->stream)) return rc;
    launch_quality_out(QualityOutArgs{e->d_quality_chan, rec, sum_a, sum_d, sum_n, max_epochs, n_chans, first_rx_sample, rx_step, n_fix, qp,
                                      (gpsacq_obs*)d_obs, (gpsacq_quality_info*)d_info},
                       e->stream);
    if (int rc = e->quality_t.mark(2, e->stream)) return rc;
    if (int rc = e->quality_t.finish()) return rc;
    return GPSACQ_OK;
}

extern "C" int gpsacq_quality_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                                 const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                                 uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, const gpsacq_quality_params* params,
                                                 void* d_obs, void* d_info, int sync) {
    gpsacq_quality_params qp;
    if (int rc = quality_check("gpsacq_quality_observables", e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, params, &qp)) return rc;
    if (!d_info) return fail(GPSACQ_ERR_ARG, "gpsacq_quality_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = quality_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, qp, d_obs, d_info)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_quality_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                          const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample,
                                          uint64_t rx_step, size_t n_fix, const gpsacq_quality_params* params, gpsacq_obs* obs,
                                          gpsacq_quality_info* info) {
    gpsacq_quality_params qp;
    if (int rc = quality_check("gpsacq_quality_observables", e, records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, params, &qp)) return rc;
    if (!info) return fail(GPSACQ_ERR_ARG, "gpsacq_quality_observables: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_quality_info.grow(n_obs, e->stream)) return rc;
    if (obs)
        if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload_records(e, records, max_epochs, n_epochs, n_chans)) return rc;
    if (int rc = quality_enqueue(e, e->d_obs_rec, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, qp,
                                 obs ? e->d_nav_obs.p : nullptr, e->d_quality_info))
        return rc;
    if (int rc = download(e, obs, e->d_nav_obs, n_obs)) return rc;
    if (int rc = download(e, info, e->d_quality_info, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_quality_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                               const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                               const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                               const gpsacq_smooth_params* smooth, const gpsacq_quality_params* quality, void* d_obs,
                                               void* d_info, void* d_fix, int sync) {
    gpsacq_quality_params qp;
    gpsacq_smooth_params sp;
    if (int rc = quality_check("gpsacq_fix_quality_track", e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, quality, &qp)) return rc;
    if (!eph || n_eph <= 0 || !d_fix || (smooth && !nom_words)) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_quality_track: bad argument");
    if (smooth)
        if (int rc = smooth_params("gpsacq_fix_quality_track", smooth, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = or_own(e, d_obs, e->d_nav_obs, n_obs)) return rc;
    if (int rc = or_own(e, d_info, e->d_quality_info, n_obs)) return rc;
    if (smooth) {
        if (int rc = smooth_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, nom_words, n_chans, first_rx_sample, rx_step, n_fix, sp, d_obs, nullptr)) return rc;
    } else {
        if (int rc = obs_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, d_obs)) return rc;
    }
    if (int rc = quality_enqueue(e, d_records, max_epochs, n_epochs, chans, tags, n_chans, first_rx_sample, rx_step, n_fix, qp, d_obs, d_info)) return rc;
    return gpsacq_fix_batch_device(e, eph, n_eph, d_obs, n_fix, n_chans, d_fix, sync);
}

extern "C" int gpsacq_quality_last_ms(const gpsacq_engine* e, float* acc_ms, float* out_ms) {
    if (!e || !e->quality_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_quality_last_ms: no gpsacq_quality_observables call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->quality_t.wait()) return rc;
    if (int rc = e->quality_t.elapsed(0, 1, acc_ms)) return rc;
    return e->quality_t.elapsed(1, 2, out_ms);
}

// ---- atmosphere, elevation mask and DOP (fix_kernels.hip) --------------------------------------------------------------------
extern "C" int gpsacq_iono_load(gpsacq_iono* io, const gpsacq_subframe* sf, int n) {
    if (!io || n < 0 || (n > 0 && !sf)) return fail(GPSACQ_ERR_ARG, "gpsacq_iono_load: bad argument");
    for (int k = 0; k < n; ++k) {
        const uint32_t* w = sf[k].words;
        if (ubits(w, 2, 20, 3) != 4 || ubits(w, 3, 1, 8) != 0x78) continue;  // subframe 4, data ID 01, SV/page ID 56: page 18
        io->valid = 1;
        io->tow = (int32_t)ubits(w, 2, 1, 17);
        // IS-GPS-200 Figure 20-1 sheet 8, Table 20-X
        io->alpha[0] = scaled(sbits(w, 3, 9, 8), -30);
        io->alpha[1] = scaled(sbits(w, 3, 17, 8), -27);
        io->alpha[2] = scaled(sbits(w, 4, 1, 8), -24);
        io->alpha[3] = scaled(sbits(w, 4, 9, 8), -24);
        io->beta[0] = scaled(sbits(w, 4, 17, 8), 11);
        io->beta[1] = scaled(sbits(w, 5, 1, 8), 14);
        io->beta[2] = scaled(sbits(w, 5, 9, 8), 16);
        io->beta[3] = scaled(sbits(w, 5, 17, 8), 16);
    }
    return GPSACQ_OK;
}

namespace {
constexpr double ATM_HALF_PI = 1.5707963267948966;
}

extern "C" int gpsacq_atm_default_params(const gpsacq_iono* io, gpsacq_atm_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_atm_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    if (io && io->valid)
        for (int k = 0; k < 4; ++k) p->alpha[k] = io->alpha[k], p->beta[k] = io->beta[k];
    p->elev_mask = 5.0 * (2.0 * ATM_HALF_PI) / 180.0;
    p->flags = GPSACQ_ATM_IONO | GPSACQ_ATM_TROPO;
    return GPSACQ_OK;
}

static int atm_check_params(const char* who, const gpsacq_atm_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "%s: params is NULL", who);
    if (!std::isfinite(p->elev_mask) || p->elev_mask < -ATM_HALF_PI || !(p->elev_mask < ATM_HALF_PI))
        return fail(GPSACQ_ERR_ARG, "%s: elev_mask %g outside [-pi/2, pi/2)", who, p->elev_mask);
    if (p->flags & ~(GPSACQ_ATM_IONO | GPSACQ_ATM_TROPO)) return fail(GPSACQ_ERR_ARG, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(p->alpha[k]) || !std::isfinite(p->beta[k])) return fail(GPSACQ_ERR_ARG, "%s: coefficient %d is not finite", who, k);
    return GPSACQ_OK;
}

static int atm_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, size_t n_fix,
                     int sats_per_fix, const gpsacq_atm_params* params, const void* out) {
    if (int rc = nav_check(who, e, eph, n_eph, obs, n_fix, out)) return rc;
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "%s: sats_per_fix %d outside 1 .. %d", who, sats_per_fix, GPSACQ_FIX_MAX_SATS);
    return atm_check_params(who, params);
}

extern "C" int gpsacq_sat_views_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_fix,
                                       size_t n_fix, int sats_per_fix, const gpsacq_atm_params* params, void* d_out, int sync) {
    if (int rc = atm_check("gpsacq_sat_views", e, eph, n_eph, d_obs, n_fix, sats_per_fix, params, d_out)) return rc;
    if (!d_fix) return fail(GPSACQ_ERR_ARG, "gpsacq_sat_views: bad argument");
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_nav_state}, e->stream);
    launch_sat_view(SatViewArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, e->d_nav_state, (const gpsacq_fix*)d_fix, n_obs, sats_per_fix, *params,
                                (gpsacq_sat_view*)d_out},
                    e->stream);
    HIPCHK(hipGetLastError());
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_sat_views(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, const gpsacq_fix* fix,
                                size_t n_fix, int sats_per_fix, const gpsacq_atm_params* params, gpsacq_sat_view* out) {
    if (int rc = atm_check("gpsacq_sat_views", e, eph, n_eph, obs, n_fix, sats_per_fix, params, out)) return rc;
    if (!fix) return fail(GPSACQ_ERR_ARG, "gpsacq_sat_views: bad argument");
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_sat_views", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_atm_view.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_nav_fix, fix, n_fix)) return rc;
    if (int rc = gpsacq_sat_views_device(e, eph, n_eph, e->d_nav_obs, e->d_nav_fix, n_fix, sats_per_fix, params, e->d_atm_view, 0)) return rc;
    if (int rc = download(e, out, e->d_atm_view, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_atm_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                           int sats_per_fix, const gpsacq_atm_params* params, void* d_fix, void* d_dop, void* d_views,
                                           int sync) {
    if (int rc = atm_check("gpsacq_fix_atm_batch", e, eph, n_eph, d_obs, n_fix, sats_per_fix, params, d_fix)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    if (int rc = or_own(e, d_dop, e->d_atm_dop, n_fix)) return rc;  // the kernel always writes it
    if (int rc = e->atm_t.begin(e->stream)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_nav_state}, e->stream);
    if (int rc = e->atm_t.mark(1, e->stream)) return rc;
    launch_fix_atm(FixAtmArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, e->d_nav_state, n_fix, sats_per_fix, *params, (gpsacq_fix*)d_fix,
                              (gpsacq_fix_dop*)d_dop},
                   e->stream);
    if (int rc = e->atm_t.mark(2, e->stream)) return rc;
    if (d_views)
        launch_sat_view(SatViewArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, e->d_nav_state, (const gpsacq_fix*)d_fix, n_obs, sats_per_fix,
                                    *params, (gpsacq_sat_view*)d_views},
                        e->stream);
    if (int rc = e->atm_t.mark(3, e->stream)) return rc;
    if (int rc = e->atm_t.finish()) return rc;
    e->atm_views = d_views != nullptr;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_atm_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_fix,
                                    int sats_per_fix, const gpsacq_atm_params* params, gpsacq_fix* fix_out, gpsacq_fix_dop* dop_out,
                                    gpsacq_sat_view* views_out) {
    if (int rc = atm_check("gpsacq_fix_atm_batch", e, eph, n_eph, obs, n_fix, sats_per_fix, params, fix_out)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_fix_atm_batch", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_nav_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_atm_dop.grow(n_fix, e->stream)) return rc;
    if (views_out)
        if (int rc = e->d_atm_view.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = gpsacq_fix_atm_batch_device(e, eph, n_eph, e->d_nav_obs, n_fix, sats_per_fix, params, e->d_nav_fix, e->d_atm_dop,
                                             views_out ? e->d_atm_view.p : nullptr, 0))
        return rc;
    if (int rc = download(e, fix_out, e->d_nav_fix, n_fix)) return rc;
    if (int rc = download(e, dop_out, e->d_atm_dop, n_fix)) return rc;
    if (int rc = download(e, views_out, e->d_atm_view, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_atm_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* fix_atm_ms, float* sat_view_ms) {
    if (!e || !e->atm_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_atm_last_ms: no gpsacq_fix_atm_batch call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->atm_t.wait()) return rc;
    if (int rc = e->atm_t.elapsed(0, 1, sat_state_ms)) return rc;
    if (int rc = e->atm_t.elapsed(1, 2, fix_atm_ms)) return rc;
    if (sat_view_ms) *sat_view_ms = 0.f;  // k_sat_view ran only where the call asked for views
    return e->atm_views ? e->atm_t.elapsed(2, 3, sat_view_ms) : GPSACQ_OK;
}

// ---- fix integrity: residual test and single-satellite exclusion (fix_kernels.hip) -----------------------------------------------
namespace {
// upper tail of the chi-square distribution at d degrees of freedom, the closed form for integer d
double chi2_tail(int d, double x) {
    const double h = 0.5 * x;
    double sum = 0.0;
    if (d % 2 == 0) {
        double term = 1.0;  // h^j / j!
        for (int j = 0; j < d / 2; ++j) {
            sum += term;
            term *= h / (double)(j + 1);
        }
        return std::exp(-h) * sum;
    }
    for (int j = 0; j < (d - 1) / 2; ++j) sum += std::pow(h, j + 0.5) / std::tgamma(j + 1.5);
    return std::erfc(std::sqrt(h)) + std::exp(-h) * sum;
}
}  // namespace

extern "C" int gpsacq_raim_default_params(double sigma_m, double p_fa, gpsacq_raim_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_raim_default_params: null argument");
    if (!std::isfinite(sigma_m) || !(sigma_m > 0.0)) return fail(GPSACQ_ERR_ARG, "gpsacq_raim_default_params: sigma_m %g (must be finite and > 0)", sigma_m);
    if (!(p_fa >= 1e-15) || !(p_fa <= 0.5)) return fail(GPSACQ_ERR_ARG, "gpsacq_raim_default_params: p_fa %g outside [1e-15, 0.5]", p_fa);
    std::memset(p, 0, sizeof *p);
    p->sigma_m = sigma_m;
    p->p_fa = p_fa;
    for (int d = 1; d <= GPSACQ_RAIM_MAX_DOF; ++d) {
        double lo = 0.0, hi = 4000.0;  // the tail falls from 1 to 0 in between
        for (int k = 0; k < 200; ++k) {
            const double mid = 0.5 * (lo + hi);
            if (chi2_tail(d, mid) > p_fa) lo = mid;
            else hi = mid;
        }
        p->threshold[d - 1] = 0.5 * (lo + hi);
    }
    p->exclude = 1;
    return GPSACQ_OK;
}

// the raim parameters of gpsacq_fix_raim_batch* and gpsacq_coarse_raim_batch*
static int raim_params_check(const char* who, const gpsacq_raim_params* rp) {
    if (!rp) return fail(GPSACQ_ERR_ARG, "%s: raim params is NULL", who);
    if (!std::isfinite(rp->sigma_m) || !(rp->sigma_m > 0.0)) return fail(GPSACQ_ERR_ARG, "%s: sigma_m %g (must be finite and > 0)", who, rp->sigma_m);
    for (int k = 0; k < GPSACQ_RAIM_MAX_DOF; ++k)
        if (!std::isfinite(rp->threshold[k]) || !(rp->threshold[k] > 0.0))
            return fail(GPSACQ_ERR_ARG, "%s: threshold %d is %g (must be finite and > 0)", who, k, rp->threshold[k]);
    if (rp->exclude != 0 && rp->exclude != 1) return fail(GPSACQ_ERR_ARG, "%s: exclude %d (must be 0 or 1)", who, (int)rp->exclude);
    return GPSACQ_OK;
}

static int raim_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, size_t n_fix,
                      int sats_per_fix, const gpsacq_atm_params* atm_params, const gpsacq_raim_params* rp, const void* fix, const void* raim) {
    if (int rc = atm_check(who, e, eph, n_eph, obs, n_fix, sats_per_fix, atm_params, fix)) return rc;
    if (!raim) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    return raim_params_check(who, rp);
}

extern "C" int gpsacq_fix_raim_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                            int sats_per_fix, const gpsacq_atm_params* atm_params, const gpsacq_raim_params* raim_params,
                                            void* d_fix, void* d_dop, void* d_raim, int sync) {
    if (int rc = raim_check("gpsacq_fix_raim_batch", e, eph, n_eph, d_obs, n_fix, sats_per_fix, atm_params, raim_params, d_fix, d_raim)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_nav_state.grow(n_obs, e->stream)) return rc;
    if (int rc = e->d_raim_rows.grow(n_fix, e->stream)) return rc;
    if (int rc = or_own(e, d_dop, e->d_atm_dop, n_fix)) return rc;  // the kernels always write it
    const RaimArgs args{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, e->d_nav_state, n_fix, sats_per_fix, *atm_params, *raim_params,
                        (gpsacq_fix*)d_fix, (gpsacq_fix_dop*)d_dop, (gpsacq_fix_raim*)d_raim, e->d_raim_rows};
    if (int rc = e->raim_t.begin(e->stream)) return rc;
    launch_sat_state(SatStateArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, n_obs, e->d_nav_state}, e->stream);
    if (int rc = e->raim_t.mark(1, e->stream)) return rc;
    launch_raim_detect(args, e->stream);
    if (int rc = e->raim_t.mark(2, e->stream)) return rc;
    launch_raim_exclude(args, e->stream);  // always: which rows were flagged is known on the device only
    if (int rc = e->raim_t.mark(3, e->stream)) return rc;
    if (int rc = e->raim_t.finish()) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_raim_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_fix,
                                     int sats_per_fix, const gpsacq_atm_params* atm_params, const gpsacq_raim_params* raim_params,
                                     gpsacq_fix* fix_out, gpsacq_fix_dop* dop_out, gpsacq_fix_raim* raim_out) {
    if (int rc = raim_check("gpsacq_fix_raim_batch", e, eph, n_eph, obs, n_fix, sats_per_fix, atm_params, raim_params, fix_out, raim_out)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_fix_raim_batch", obs, n_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_nav_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_atm_dop.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_raim.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = gpsacq_fix_raim_batch_device(e, eph, n_eph, e->d_nav_obs, n_fix, sats_per_fix, atm_params, raim_params, e->d_nav_fix,
                                              e->d_atm_dop, e->d_raim, 0))
        return rc;
    if (int rc = download(e, fix_out, e->d_nav_fix, n_fix)) return rc;
    if (int rc = download(e, dop_out, e->d_atm_dop, n_fix)) return rc;
    if (int rc = download(e, raim_out, e->d_raim, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fix_raim_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* detect_ms, float* exclude_ms) {
    if (!e || !e->raim_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_fix_raim_last_ms: no gpsacq_fix_raim_batch call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->raim_t.wait()) return rc;
    if (int rc = e->raim_t.elapsed(0, 1, sat_state_ms)) return rc;
    if (int rc = e->raim_t.elapsed(1, 2, detect_ms)) return rc;
    return e->raim_t.elapsed(2, 3, exclude_ms);
}

// ---- coarse-time fixes: positions from code phases alone (coarse_kernels.hip) ----------------------------------------------------
extern "C" int gpsacq_coarse_default_params(gpsacq_coarse_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->rms_max_m = 2.99792458e8 / 1.023e6;  // one C/A chip
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int coarse_params(const char* who, const gpsacq_coarse_params* params, gpsacq_coarse_params* out) {
    if (!params) return gpsacq_coarse_default_params(out);
    *out = *params;
    if (!std::isfinite(out->rms_max_m) || !(out->rms_max_m > 0.0)) return fail(GPSACQ_ERR_ARG, "%s: rms_max_m %g (must be finite and > 0)", who, out->rms_max_m);
    return GPSACQ_OK;
}

static int coarse_fix_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, const void* prior,
                            size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params, const void* fix, const void* info,
                            const void* obs_out, gpsacq_coarse_params* checked) {
    if (int rc = nav_check(who, e, eph, n_eph, obs, n_fix, fix)) return rc;
    if (!prior || !info) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "%s: sats_per_fix %d outside 1 .. %d", who, sats_per_fix, GPSACQ_FIX_MAX_SATS);
    if (obs_out == obs) return fail(GPSACQ_ERR_ARG, "%s: obs_out must not be obs", who);
    return coarse_params(who, params, checked);
}

// the host forms can read their priors: one that names no place or no instant of the week is an argument error
static int coarse_check_priors(const char* who, const gpsacq_coarse_prior* prior, size_t n_fix) {
    for (size_t k = 0; k < n_fix; ++k)
        if (prior[k].rx_ms < 0 || prior[k].rx_ms >= 604800000 || !std::isfinite(prior[k].x) || !std::isfinite(prior[k].y) || !std::isfinite(prior[k].z))
            return fail(GPSACQ_ERR_ARG, "%s: prior %zu is (%g, %g, %g) at rx_ms %d (must be finite, 0 <= rx_ms < 604800000)", who, k, prior[k].x,
                        prior[k].y, prior[k].z, (int)prior[k].rx_ms);
    return GPSACQ_OK;
}

static int coarse_obs_check(const char* who, const gpsacq_engine* e, const void* peaks, size_t n_fix, int n_chans, double snr_min, const void* obs) {
    if (!e || !peaks || !obs || n_fix == 0 || n_fix > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (n_chans < 1 || n_chans > GPSACQ_FIX_MAX_SATS) return fail(GPSACQ_ERR_ARG, "%s: n_chans %d outside 1 .. %d", who, n_chans, GPSACQ_FIX_MAX_SATS);
    if (!std::isfinite(snr_min)) return fail(GPSACQ_ERR_ARG, "%s: snr_min %g (must be finite)", who, snr_min);
    return GPSACQ_OK;
}

// k_coarse_obs on the engine's stream timed; every argument has been checked
static int coarse_obs_enqueue(gpsacq_engine* e, const void* d_peaks, size_t n_fix, int n_chans, double snr_min, void* d_obs) {
    return timed_stage(e->coarse_obs_t, e->stream, [&] {
        launch_coarse_obs(CoarseObsArgs{(const gpsacq_peak*)d_peaks, n_fix * (size_t)n_chans, n_chans, e->p.fs, snr_min, (gpsacq_obs*)d_obs}, e->stream);
    });
}

// the ephemerides up, then k_coarse_fix timed; every argument has been checked
static int coarse_fix_enqueue(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_prior, size_t n_fix,
                              int sats_per_fix, const gpsacq_coarse_params& cp, void* d_fix, void* d_info, void* d_obs_out) {
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = or_own(e, d_obs_out, e->d_coarse_work, n_fix * (size_t)sats_per_fix)) return rc;  // the whole milliseconds live somewhere
    return timed_stage(e->coarse_fix_t, e->stream, [&] {
        launch_coarse_fix(CoarseFixArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, (const gpsacq_coarse_prior*)d_prior, n_fix, sats_per_fix, cp,
                                        (gpsacq_fix*)d_fix, (gpsacq_coarse_info*)d_info, (gpsacq_obs*)d_obs_out},
                          e->stream);
    });
}

extern "C" int gpsacq_coarse_obs_device(gpsacq_engine* e, const void* d_peaks, size_t n_fix, int n_chans, double snr_min, void* d_obs, int sync) {
    if (int rc = coarse_obs_check("gpsacq_coarse_obs", e, d_peaks, n_fix, n_chans, snr_min, d_obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = coarse_obs_enqueue(e, d_peaks, n_fix, n_chans, snr_min, d_obs)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_obs(gpsacq_engine* e, const gpsacq_peak* peaks, size_t n_fix, int n_chans, double snr_min, gpsacq_obs* obs) {
    if (int rc = coarse_obs_check("gpsacq_coarse_obs", e, peaks, n_fix, n_chans, snr_min, obs)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_coarse_obs.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_coarse_peaks, peaks, n_obs)) return rc;
    if (int rc = coarse_obs_enqueue(e, e->d_coarse_peaks, n_fix, n_chans, snr_min, e->d_coarse_obs)) return rc;
    if (int rc = download(e, obs, e->d_coarse_obs, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_prior,
                                              size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params, void* d_fix, void* d_info,
                                              void* d_obs_out, int sync) {
    gpsacq_coarse_params cp;
    if (int rc = coarse_fix_check("gpsacq_coarse_fix_batch", e, eph, n_eph, d_obs, d_prior, n_fix, sats_per_fix, params, d_fix, d_info, d_obs_out, &cp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, sats_per_fix, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs,
                                       const gpsacq_coarse_prior* prior, size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params,
                                       gpsacq_fix* fix_out, gpsacq_coarse_info* info_out, gpsacq_obs* obs_out) {
    gpsacq_coarse_params cp;
    if (int rc = coarse_fix_check("gpsacq_coarse_fix_batch", e, eph, n_eph, obs, prior, n_fix, sats_per_fix, params, fix_out, info_out, obs_out, &cp))
        return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_coarse_fix_batch", obs, n_obs)) return rc;
    if (int rc = coarse_check_priors("gpsacq_coarse_fix_batch", prior, n_fix)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_coarse_work.grow(n_obs, e->stream)) return rc;
    if (int rc = e->d_nav_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_coarse_info.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_coarse_prior, prior, n_fix)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, e->d_nav_obs, e->d_coarse_prior, n_fix, sats_per_fix, cp, e->d_nav_fix, e->d_coarse_info, nullptr))
        return rc;
    if (int rc = download(e, fix_out, e->d_nav_fix, n_fix)) return rc;
    if (int rc = download(e, info_out, e->d_coarse_info, n_fix)) return rc;
    if (int rc = download(e, obs_out, e->d_coarse_work, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_peaks, size_t n_fix,
                                              int n_chans, double snr_min, const void* d_prior, const gpsacq_coarse_params* params, void* d_obs,
                                              void* d_fix, void* d_info, void* d_obs_out, int sync) {
    if (int rc = coarse_obs_check("gpsacq_coarse_fix_peaks", e, d_peaks, n_fix, n_chans, snr_min, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_prior || !d_info) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_peaks: bad argument");
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_peaks: obs_out must not be obs");
    gpsacq_coarse_params cp;
    if (int rc = coarse_params("gpsacq_coarse_fix_peaks", params, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_fix * (size_t)n_chans)) return rc;
    if (int rc = coarse_obs_enqueue(e, d_peaks, n_fix, n_chans, snr_min, d_obs)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_last_ms(const gpsacq_engine* e, float* obs_ms, float* fix_ms) {
    if (!e || (!e->coarse_obs_t.ran() && !e->coarse_fix_t.ran())) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_last_ms: no gpsacq_coarse call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->coarse_obs_t, obs_ms)) return rc;
    return stage_ms(e->coarse_fix_t, fix_ms);
}

// ---- coarse-time fix integrity: residual test and one-satellite exclusion (coarse_kernels.hip) -----------------------------------
static int coarse_raim_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, const void* prior,
                             size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params, const gpsacq_raim_params* rp, const void* fix,
                             const void* info, const void* obs_out, const void* raim, gpsacq_coarse_params* checked) {
    if (int rc = coarse_fix_check(who, e, eph, n_eph, obs, prior, n_fix, sats_per_fix, params, fix, info, obs_out, checked)) return rc;
    if (!raim) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    return raim_params_check(who, rp);
}

extern "C" int gpsacq_coarse_raim_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_prior,
                                               size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* coarse_par,
                                               const gpsacq_raim_params* raim_params, void* d_fix, void* d_info, void* d_obs_out, void* d_raim,
                                               int sync) {
    gpsacq_coarse_params cp;
    if (int rc = coarse_raim_check("gpsacq_coarse_raim_batch", e, eph, n_eph, d_obs, d_prior, n_fix, sats_per_fix, coarse_par, raim_params, d_fix, d_info,
                                   d_obs_out, d_raim, &cp))
        return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    void* d_work = d_obs_out;
    if (int rc = or_own(e, d_work, e->d_coarse_work, n_obs)) return rc;  // FULL's whole milliseconds live somewhere
    if (int rc = e->d_coarse_cand.grow(n_obs * (size_t)sats_per_fix, e->stream)) return rc;
    const CoarseFixArgs full{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, (const gpsacq_coarse_prior*)d_prior, n_fix, sats_per_fix, cp,
                             (gpsacq_fix*)d_fix, (gpsacq_coarse_info*)d_info, (gpsacq_obs*)d_work};
    if (int rc = e->coarse_raim_t.begin(e->stream)) return rc;
    launch_coarse_fix(full, e->stream);
    if (int rc = e->coarse_raim_t.mark(1, e->stream)) return rc;
    // always: which rows were flagged is known on the device only
    launch_coarse_exclude(CoarseRaimArgs{full, *raim_params, (gpsacq_fix_raim*)d_raim, e->d_coarse_cand, (gpsacq_obs*)d_obs_out}, e->stream);
    if (int rc = e->coarse_raim_t.mark(2, e->stream)) return rc;
    if (int rc = e->coarse_raim_t.finish()) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_raim_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs,
                                        const gpsacq_coarse_prior* prior, size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* coarse_par,
                                        const gpsacq_raim_params* raim_params, gpsacq_fix* fix_out, gpsacq_coarse_info* info_out,
                                        gpsacq_obs* obs_out, gpsacq_fix_raim* raim_out) {
    gpsacq_coarse_params cp;
    if (int rc = coarse_raim_check("gpsacq_coarse_raim_batch", e, eph, n_eph, obs, prior, n_fix, sats_per_fix, coarse_par, raim_params, fix_out, info_out,
                                   obs_out, raim_out, &cp))
        return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    if (int rc = nav_check_weights("gpsacq_coarse_raim_batch", obs, n_obs)) return rc;
    if (int rc = coarse_check_priors("gpsacq_coarse_raim_batch", prior, n_fix)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_coarse_work.grow(n_obs, e->stream)) return rc;
    if (int rc = e->d_nav_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_coarse_info.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_raim.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_coarse_prior, prior, n_fix)) return rc;
    // d_coarse_work as the caller's obs_out: the winning lane of an excluded row copies its observations there
    if (int rc = gpsacq_coarse_raim_batch_device(e, eph, n_eph, e->d_nav_obs, e->d_coarse_prior, n_fix, sats_per_fix, &cp, raim_params, e->d_nav_fix,
                                                 e->d_coarse_info, e->d_coarse_work, e->d_raim, 0))
        return rc;
    if (int rc = download(e, fix_out, e->d_nav_fix, n_fix)) return rc;
    if (int rc = download(e, info_out, e->d_coarse_info, n_fix)) return rc;
    if (int rc = download(e, obs_out, e->d_coarse_work, n_obs)) return rc;
    if (int rc = download(e, raim_out, e->d_raim, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_raim_last_ms(const gpsacq_engine* e, float* fix_ms, float* exclude_ms) {
    if (!e || !e->coarse_raim_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_raim_last_ms: no gpsacq_coarse_raim_batch call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->coarse_raim_t.wait()) return rc;
    if (int rc = e->coarse_raim_t.elapsed(0, 1, fix_ms)) return rc;
    return e->coarse_raim_t.elapsed(1, 2, exclude_ms);
}

// ---- fine code phases: search peaks refined below a sample (refine_kernels.hip) --------------------------------------------------
extern "C" int gpsacq_refine_default_params(gpsacq_refine_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_refine_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->blocks = 16;
    p->min_segments = 1;
    p->half_spacing_chips = 0.25;
    p->snr_min = 25.0;  // the threshold of the search, c/search_offline.cpp:248
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int refine_params(const char* who, const gpsacq_refine_params* params, gpsacq_refine_params* out) {
    if (!params) return gpsacq_refine_default_params(out);
    *out = *params;
    if (out->blocks < 1 || out->blocks > 64) return fail(GPSACQ_ERR_ARG, "%s: blocks %d outside 1 .. 64", who, (int)out->blocks);
    if (out->min_segments < 1) return fail(GPSACQ_ERR_ARG, "%s: min_segments %d (must be >= 1)", who, (int)out->min_segments);
    if (!(out->half_spacing_chips >= 1.0 / 64 && out->half_spacing_chips <= 0.5))
        return fail(GPSACQ_ERR_ARG, "%s: half_spacing_chips %g outside [1/64, 0.5]", who, out->half_spacing_chips);
    if (!std::isfinite(out->snr_min)) return fail(GPSACQ_ERR_ARG, "%s: snr_min %g (must be finite)", who, out->snr_min);
    return GPSACQ_OK;
}

// the engines the kernels that go back to the capture serve
static int capture_engine_check(const char* who, const gpsacq_engine* e) {
    if (e->nlags > 65535) return fail(GPSACQ_ERR_UNSUPPORTED, "%s: %d samples per millisecond (the packed counts hold 65535)", who, e->nlags);
    if (1.023e6 / e->p.fs + 1.0 / 1540.0 > REFINE_MAX_CHIPS_PER_SAMPLE)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: fs = %g Hz is fewer than %.2f samples per chip (a word's chips leave the kernel's window)", who, e->p.fs,
                    1.0 / REFINE_MAX_CHIPS_PER_SAMPLE);
    return GPSACQ_OK;
}

// the capture, the peaks, the output and the engine of a kernel that goes back to the capture (k_refine, k_fine_dop)
static int capture_check(const char* who, const gpsacq_engine* e, const void* bits, size_t n_bytes, size_t stride, const void* peaks, size_t n_tasks,
                         const void* out) {
    if (!e || !bits || !peaks || !out || n_bytes == 0 || n_tasks == 0 || n_tasks > 0x7fffffffu) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (stride < 5000 || stride > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: stride %zu outside 5000 .. 2^31", who, stride);
    if (n_bytes > ((size_t)1 << 56)) return fail(GPSACQ_ERR_ARG, "%s: n_bytes %zu", who, n_bytes);
    return capture_engine_check(who, e);
}

static int refine_check(const char* who, const gpsacq_engine* e, const void* bits, size_t n_bytes, size_t stride, const void* peaks, size_t n_tasks,
                        const gpsacq_refine_params* params, const void* fine, gpsacq_refine_params* checked) {
    if (int rc = capture_check(who, e, bits, n_bytes, stride, peaks, n_tasks, fine)) return rc;
    return refine_params(who, params, checked);
}

// what every kernel on a 1-bit capture is told alike: the capture, its tasks and peaks, the chip table and the engine's grid
static BitCaptureArgs capture_args(const gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                                   size_t n_tasks) {
    const uint32_t lead = (uint32_t)((uintptr_t)d_bits & 3u);  // the kernel loads whole words from the aligned address below
    const bool ref_grid = e->sub == 1 && e->dstride == 1;       // as gpsacq_handoff_engine
    BitCaptureArgs c{};
    c.words = (const uint32_t*)((uintptr_t)d_bits - lead);
    c.n_bytes = n_bytes + lead;
    c.lead = lead;
    c.stride = stride;
    c.tasks = (const gpsacq_task*)d_tasks;
    c.peaks = (const gpsacq_peak*)d_peaks;
    c.n_tasks = n_tasks;
    c.chips = e->d_track_chips;
    c.fc = e->p.fc, c.fs = e->p.fs;
    c.step_hz = ref_grid ? 0.0 : e->p.fs / N_FFT * e->dstride / e->sub;
    c.spm = e->nlags;
    return c;
}

// k_refine on the engine's stream timed; every argument has been checked
static int refine_enqueue(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                          size_t n_tasks, const gpsacq_refine_params& rp, void* d_fine) {
    if (int rc = ensure_track_chips(e)) return rc;
    RefineArgs a{};
    a.c = capture_args(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks);
    a.p = rp;
    a.out = (gpsacq_fine*)d_fine;
    return timed_stage(e->refine_t, e->stream, [&] { launch_refine(a, e->stream); });
}

// k_coarse_obs_fine timed; every argument has been checked
static int coarse_obs_fine_enqueue(gpsacq_engine* e, const void* d_peaks, const void* d_fine, size_t n_fix, int n_chans, double snr_min, void* d_obs) {
    return timed_stage(e->refine_obs_t, e->stream, [&] {
        launch_coarse_obs_fine(CoarseObsFineArgs{(const gpsacq_peak*)d_peaks, (const gpsacq_fine*)d_fine, n_fix * (size_t)n_chans, n_chans, e->p.fs, snr_min,
                                                 (gpsacq_obs*)d_obs},
                               e->stream);
    });
}

extern "C" int gpsacq_refine_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                                    size_t n_tasks, const gpsacq_refine_params* params, void* d_fine, int sync) {
    gpsacq_refine_params rp;
    if (int rc = refine_check("gpsacq_refine", e, d_bits, n_bytes, stride, d_peaks, n_tasks, params, d_fine, &rp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = refine_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_refine(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks, const gpsacq_peak* peaks,
                             size_t n_tasks, const gpsacq_refine_params* params, gpsacq_fine* fine_out) {
    gpsacq_refine_params rp;
    if (int rc = refine_check("gpsacq_refine", e, bits, n_bytes, stride, peaks, n_tasks, params, fine_out, &rp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_fine.grow(n_tasks, e->stream)) return rc;
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    if (int rc = upload(e, e->d_refine_bits, bits, n_bytes)) return rc;
    if (int rc = upload(e, e->d_refine_peaks, peaks, n_tasks)) return rc;
    if (int rc = refine_enqueue(e, e->d_refine_bits, n_bytes, stride, tasks ? e->d_refine_tasks.p : nullptr, e->d_refine_peaks, n_tasks, rp, e->d_fine))
        return rc;
    if (int rc = download(e, fine_out, e->d_fine, n_tasks)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_obs_fine_device(gpsacq_engine* e, const void* d_peaks, const void* d_fine, size_t n_fix, int n_chans, double snr_min,
                                             void* d_obs, int sync) {
    if (int rc = coarse_obs_check("gpsacq_coarse_obs_fine", e, d_peaks, n_fix, n_chans, snr_min, d_obs)) return rc;
    if (!d_fine) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_obs_fine: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, snr_min, d_obs)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_obs_fine(gpsacq_engine* e, const gpsacq_peak* peaks, const gpsacq_fine* fine, size_t n_fix, int n_chans, double snr_min,
                                      gpsacq_obs* obs) {
    if (int rc = coarse_obs_check("gpsacq_coarse_obs_fine", e, peaks, n_fix, n_chans, snr_min, obs)) return rc;
    if (!fine) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_obs_fine: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_coarse_obs.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_refine_peaks, peaks, n_obs)) return rc;
    if (int rc = upload(e, e->d_fine, fine, n_obs)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, e->d_refine_peaks, e->d_fine, n_fix, n_chans, snr_min, e->d_coarse_obs)) return rc;
    if (int rc = download(e, obs, e->d_coarse_obs, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_fine_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes, size_t stride,
                                             const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                             const gpsacq_refine_params* refine_par, const void* d_prior, const gpsacq_coarse_params* params,
                                             void* d_fine, void* d_obs, void* d_fix, void* d_info, void* d_obs_out, int sync) {
    if (int rc = coarse_obs_check("gpsacq_coarse_fix_fine", e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_prior || !d_info) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_fine: bad argument");
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_fine: obs_out must not be obs");
    const size_t n_tasks = n_fix * (size_t)n_chans;
    gpsacq_refine_params rp;
    if (int rc = refine_check("gpsacq_coarse_fix_fine", e, d_bits, n_bytes, stride, d_peaks, n_tasks, refine_par, d_fix, &rp)) return rc;
    gpsacq_coarse_params cp;
    if (int rc = coarse_params("gpsacq_coarse_fix_fine", params, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = refine_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_refine_last_ms(const gpsacq_engine* e, float* refine_ms, float* obs_ms) {
    if (!e || (!e->refine_t.ran() && !e->refine_obs_t.ran())) return fail(GPSACQ_ERR_ARG, "gpsacq_refine_last_ms: no gpsacq_refine call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->refine_t, refine_ms)) return rc;
    return stage_ms(e->refine_obs_t, obs_ms);
}

// ---- snapshot signal quality: C/N0 and weights of fine code phases (snapq_kernels.hip) -----------------------------------------
extern "C" int gpsacq_snap_quality_default_params(gpsacq_snap_quality_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_snap_quality_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->min_segments = 1;
    p->cn0_min_lin = 500.0;
    p->cn0_ref_lin = std::pow(10.0, 4.35);
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int snap_quality_params(const char* who, const gpsacq_snap_quality_params* params, gpsacq_snap_quality_params* out) {
    if (!params) return gpsacq_snap_quality_default_params(out);
    *out = *params;
    if (out->min_segments < 1) return fail(GPSACQ_ERR_ARG, "%s: min_segments %d (must be >= 1)", who, (int)out->min_segments);
    if (!(out->cn0_min_lin >= 0.0) || !std::isfinite(out->cn0_min_lin)) return fail(GPSACQ_ERR_ARG, "%s: cn0_min_lin %g must be finite and >= 0", who, out->cn0_min_lin);
    if (!(out->cn0_ref_lin > 0.0) || !std::isfinite(out->cn0_ref_lin)) return fail(GPSACQ_ERR_ARG, "%s: cn0_ref_lin %g must be finite and > 0", who, out->cn0_ref_lin);
    return GPSACQ_OK;
}

static int snap_quality_check(const char* who, const gpsacq_engine* e, const void* fine, size_t n_fix, int n_chans,
                              const gpsacq_snap_quality_params* params, const void* info, gpsacq_snap_quality_params* checked) {
    if (!e || !fine || !info || n_fix == 0 || n_fix > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (n_chans < 1 || n_chans > GPSACQ_FIX_MAX_SATS) return fail(GPSACQ_ERR_ARG, "%s: n_chans %d outside 1 .. %d", who, n_chans, GPSACQ_FIX_MAX_SATS);
    return snap_quality_params(who, params, checked);
}

// k_snap_quality on the engine's stream timed; every argument has been checked
static int snap_quality_enqueue(gpsacq_engine* e, const void* d_fine, size_t n_fix, int n_chans, const gpsacq_snap_quality_params& qp, void* d_obs,
                                void* d_info) {
    return timed_stage(e->snapq_t, e->stream, [&] {
        launch_snap_quality(SnapQualityArgs{(const gpsacq_fine*)d_fine, n_fix * (size_t)n_chans, e->nlags, e->p.fs, qp, (gpsacq_obs*)d_obs,
                                            (gpsacq_quality_info*)d_info},
                            e->stream);
    });
}

extern "C" int gpsacq_snap_quality_device(gpsacq_engine* e, const void* d_fine, size_t n_fix, int n_chans, const gpsacq_snap_quality_params* params,
                                          void* d_obs, void* d_info, int sync) {
    gpsacq_snap_quality_params qp;
    if (int rc = snap_quality_check("gpsacq_snap_quality", e, d_fine, n_fix, n_chans, params, d_info, &qp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = snap_quality_enqueue(e, d_fine, n_fix, n_chans, qp, d_obs, d_info)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_quality(gpsacq_engine* e, const gpsacq_fine* fine, size_t n_fix, int n_chans, const gpsacq_snap_quality_params* params,
                                   gpsacq_obs* obs, gpsacq_quality_info* info) {
    gpsacq_snap_quality_params qp;
    if (int rc = snap_quality_check("gpsacq_snap_quality", e, fine, n_fix, n_chans, params, info, &qp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_snapq_info.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_fine, fine, n_obs)) return rc;
    if (obs)
        if (int rc = upload(e, e->d_coarse_obs, (const gpsacq_obs*)obs, n_obs)) return rc;
    if (int rc = snap_quality_enqueue(e, e->d_fine, n_fix, n_chans, qp, obs ? e->d_coarse_obs.p : nullptr, e->d_snapq_info)) return rc;
    if (int rc = download(e, obs, e->d_coarse_obs, n_obs)) return rc;
    if (int rc = download(e, info, e->d_snapq_info, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_quality_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes,
                                                size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                const gpsacq_refine_params* refine_par, const gpsacq_snap_quality_params* quality_par,
                                                const void* d_prior, const gpsacq_coarse_params* params, void* d_fine, void* d_obs, void* d_qinfo,
                                                void* d_fix, void* d_info, void* d_obs_out, int sync) {
    if (int rc = coarse_obs_check("gpsacq_coarse_fix_quality", e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_prior || !d_info) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_quality: bad argument");
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "gpsacq_coarse_fix_quality: obs_out must not be obs");
    const size_t n_tasks = n_fix * (size_t)n_chans;
    gpsacq_refine_params rp;
    if (int rc = refine_check("gpsacq_coarse_fix_quality", e, d_bits, n_bytes, stride, d_peaks, n_tasks, refine_par, d_fix, &rp)) return rc;
    gpsacq_snap_quality_params qp;
    if (int rc = snap_quality_params("gpsacq_coarse_fix_quality", quality_par, &qp)) return rc;
    gpsacq_coarse_params cp;
    if (int rc = coarse_params("gpsacq_coarse_fix_quality", params, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = or_own(e, d_qinfo, e->d_snapq_info, n_tasks)) return rc;
    if (int rc = refine_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = snap_quality_enqueue(e, d_fine, n_fix, n_chans, qp, d_obs, d_qinfo)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_quality_last_ms(const gpsacq_engine* e, float* ms) {
    if (!e || !e->snapq_t.ran()) return fail(GPSACQ_ERR_ARG, "gpsacq_snap_quality_last_ms: no gpsacq_snap_quality call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    return stage_ms(e->snapq_t, ms);
}

// ---- cold snapshot fixes: fine Doppler and a Doppler-only position solver (doppler_kernels.hip) ----------------------------------
extern "C" int gpsacq_dopfine_default_params(gpsacq_dopfine_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_dopfine_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->blocks = 16;
    p->min_segments = 2;
    p->snr_min = 25.0;  // the threshold of the search, as gpsacq_refine_default_params
    p->coherence_min = 0.0;
    return GPSACQ_OK;
}

extern "C" int gpsacq_doppler_fix_default_params(gpsacq_doppler_fix_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_doppler_fix_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->rms_max_mps = 3.0;  // three times the largest rms of 2048 measured blocks (0.72 m/s), rounded up: include/gpsacq.h
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked against the bounds and the engine (OVERFLOW, and the LDS of k_fine_dop)
static int dopfine_params(const char* who, const gpsacq_engine* e, const gpsacq_dopfine_params* params, gpsacq_dopfine_params* out) {
    if (!params) {
        if (int rc = gpsacq_dopfine_default_params(out)) return rc;
    } else {
        *out = *params;
    }
    if (out->blocks < 1 || out->blocks > 64) return fail(GPSACQ_ERR_ARG, "%s: blocks %d outside 1 .. 64", who, (int)out->blocks);
    if (out->min_segments < 2) return fail(GPSACQ_ERR_ARG, "%s: min_segments %d (must be >= 2)", who, (int)out->min_segments);
    if (!std::isfinite(out->snr_min)) return fail(GPSACQ_ERR_ARG, "%s: snr_min %g (must be finite)", who, out->snr_min);
    if (!std::isfinite(out->coherence_min) || out->coherence_min < 0.0)
        return fail(GPSACQ_ERR_ARG, "%s: coherence_min %g (must be finite and >= 0)", who, out->coherence_min);
    const unsigned __int128 spm = (unsigned __int128)e->nlags;  // 1137 .. 65535 after capture_check
    if ((unsigned __int128)out->blocks * 160000u * spm * spm * spm >= (unsigned __int128)1 << 63)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: %d blocks of %d samples per millisecond (the lag sums could leave 63 bits)", who, (int)out->blocks, e->nlags);
    if ((uint64_t)out->blocks * 40000u / (uint64_t)e->nlags > (uint64_t)DOP_MAX_SEGMENTS)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: a window of more than %d segments", who, DOP_MAX_SEGMENTS);
    return GPSACQ_OK;
}

static int doppler_fix_params(const char* who, const gpsacq_doppler_fix_params* params, gpsacq_doppler_fix_params* out) {
    if (!params) return gpsacq_doppler_fix_default_params(out);
    *out = *params;
    if (!std::isfinite(out->rms_max_mps) || !(out->rms_max_mps > 0.0))
        return fail(GPSACQ_ERR_ARG, "%s: rms_max_mps %g (must be finite and > 0)", who, out->rms_max_mps);
    return GPSACQ_OK;
}

static int doppler_fix_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* obs, const void* rate_obs,
                             const void* rx_ms, size_t n_fix, int sats_per_fix, const gpsacq_doppler_fix_params* params, const void* fix,
                             gpsacq_doppler_fix_params* checked) {
    if (int rc = nav_check(who, e, eph, n_eph, obs, n_fix, fix)) return rc;
    if (!rate_obs || !rx_ms) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (sats_per_fix < 1 || sats_per_fix > GPSACQ_FIX_MAX_SATS)
        return fail(GPSACQ_ERR_ARG, "%s: sats_per_fix %d outside 1 .. %d", who, sats_per_fix, GPSACQ_FIX_MAX_SATS);
    return doppler_fix_params(who, params, checked);
}

// k_fine_dop on the engine's stream timed; every argument has been checked
static int fine_dop_enqueue(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                            size_t n_tasks, const gpsacq_dopfine_params& dp, void* d_dopfine) {
    if (int rc = ensure_track_chips(e)) return rc;
    FineDopArgs a{};
    a.c = capture_args(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks);
    a.p = dp;
    a.out = (gpsacq_dopfine*)d_dopfine;
    return timed_stage(e->dop_fine_t, e->stream, [&] { launch_fine_dop(a, e->stream); });
}

// k_rate_obs_fine timed; every argument has been checked
static int rate_obs_fine_enqueue(gpsacq_engine* e, const void* d_peaks, const void* d_dopfine, size_t n_fix, int n_chans, double snr_min,
                                 void* d_rate_obs) {
    return timed_stage(e->dop_obs_t, e->stream, [&] {
        launch_rate_obs_fine(RateObsFineArgs{(const gpsacq_peak*)d_peaks, (const gpsacq_dopfine*)d_dopfine, n_fix * (size_t)n_chans, snr_min,
                                             (gpsacq_rate_obs*)d_rate_obs},
                             e->stream);
    });
}

// the ephemerides up, then k_doppler_fix timed; every argument has been checked
static int doppler_fix_enqueue(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_rate_obs, const void* d_rx_ms,
                               size_t n_fix, int sats_per_fix, const gpsacq_doppler_fix_params& fp, void* d_fix, void* d_prior) {
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    if (int rc = e->d_dop_tau.grow(n_fix * (size_t)sats_per_fix, e->stream)) return rc;
    return timed_stage(e->dop_fix_t, e->stream, [&] {
        launch_doppler_fix(DopplerFixArgs{e->d_nav_eph, n_eph, (const gpsacq_obs*)d_obs, (const gpsacq_rate_obs*)d_rate_obs, (const int32_t*)d_rx_ms, n_fix,
                                          sats_per_fix, fp, e->d_dop_tau, (gpsacq_doppler_fix*)d_fix, (gpsacq_coarse_prior*)d_prior},
                           e->stream);
    });
}

extern "C" int gpsacq_fine_doppler_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                                          size_t n_tasks, const gpsacq_dopfine_params* params, void* d_dopfine, int sync) {
    gpsacq_dopfine_params dp;
    if (int rc = capture_check("gpsacq_fine_doppler", e, d_bits, n_bytes, stride, d_peaks, n_tasks, d_dopfine)) return rc;
    if (int rc = dopfine_params("gpsacq_fine_doppler", e, params, &dp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = fine_dop_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, dp, d_dopfine)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fine_doppler(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks,
                                   const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_dopfine_params* params, gpsacq_dopfine* dopfine_out) {
    gpsacq_dopfine_params dp;
    if (int rc = capture_check("gpsacq_fine_doppler", e, bits, n_bytes, stride, peaks, n_tasks, dopfine_out)) return rc;
    if (int rc = dopfine_params("gpsacq_fine_doppler", e, params, &dp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_dopfine.grow(n_tasks, e->stream)) return rc;
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    if (int rc = upload(e, e->d_refine_bits, bits, n_bytes)) return rc;
    if (int rc = upload(e, e->d_refine_peaks, peaks, n_tasks)) return rc;
    if (int rc = fine_dop_enqueue(e, e->d_refine_bits, n_bytes, stride, tasks ? e->d_refine_tasks.p : nullptr, e->d_refine_peaks, n_tasks, dp, e->d_dopfine))
        return rc;
    if (int rc = download(e, dopfine_out, e->d_dopfine, n_tasks)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_rate_obs_fine_device(gpsacq_engine* e, const void* d_peaks, const void* d_dopfine, size_t n_fix, int n_chans, double snr_min,
                                           void* d_rate_obs, int sync) {
    if (int rc = coarse_obs_check("gpsacq_rate_obs_fine", e, d_peaks, n_fix, n_chans, snr_min, d_rate_obs)) return rc;
    if (!d_dopfine) return fail(GPSACQ_ERR_ARG, "gpsacq_rate_obs_fine: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = rate_obs_fine_enqueue(e, d_peaks, d_dopfine, n_fix, n_chans, snr_min, d_rate_obs)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_rate_obs_fine(gpsacq_engine* e, const gpsacq_peak* peaks, const gpsacq_dopfine* dopfine, size_t n_fix, int n_chans,
                                    double snr_min, gpsacq_rate_obs* rate_obs) {
    if (int rc = coarse_obs_check("gpsacq_rate_obs_fine", e, peaks, n_fix, n_chans, snr_min, rate_obs)) return rc;
    if (!dopfine) return fail(GPSACQ_ERR_ARG, "gpsacq_rate_obs_fine: bad argument");
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_rate_obs.grow(n_obs, e->stream)) return rc;
    if (int rc = upload(e, e->d_refine_peaks, peaks, n_obs)) return rc;
    if (int rc = upload(e, e->d_dopfine, dopfine, n_obs)) return rc;
    if (int rc = rate_obs_fine_enqueue(e, e->d_refine_peaks, e->d_dopfine, n_fix, n_chans, snr_min, e->d_rate_obs)) return rc;
    if (int rc = download(e, rate_obs, e->d_rate_obs, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_doppler_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_rate_obs,
                                               const void* d_rx_ms, size_t n_fix, int sats_per_fix, const gpsacq_doppler_fix_params* params,
                                               void* d_doppler_fix, void* d_prior, int sync) {
    gpsacq_doppler_fix_params fp;
    if (int rc = doppler_fix_check("gpsacq_doppler_fix_batch", e, eph, n_eph, d_obs, d_rate_obs, d_rx_ms, n_fix, sats_per_fix, params, d_doppler_fix, &fp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = doppler_fix_enqueue(e, eph, n_eph, d_obs, d_rate_obs, d_rx_ms, n_fix, sats_per_fix, fp, d_doppler_fix, d_prior)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_doppler_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, const gpsacq_rate_obs* rate_obs,
                                        const int32_t* rx_ms, size_t n_fix, int sats_per_fix, const gpsacq_doppler_fix_params* params,
                                        gpsacq_doppler_fix* fix_out, gpsacq_coarse_prior* prior_out) {
    gpsacq_doppler_fix_params fp;
    if (int rc = doppler_fix_check("gpsacq_doppler_fix_batch", e, eph, n_eph, obs, rate_obs, rx_ms, n_fix, sats_per_fix, params, fix_out, &fp)) return rc;
    const size_t n_obs = n_fix * (size_t)sats_per_fix;
    for (size_t k = 0; k < n_obs; ++k)
        if (!(rate_obs[k].weight >= 0.0) || !std::isfinite(rate_obs[k].weight))
            return fail(GPSACQ_ERR_ARG, "gpsacq_doppler_fix_batch: rate observation %zu has weight %g (must be finite and >= 0)", k, rate_obs[k].weight);
    for (size_t k = 0; k < n_fix; ++k)
        if (rx_ms[k] < 0 || rx_ms[k] >= 604800000)
            return fail(GPSACQ_ERR_ARG, "gpsacq_doppler_fix_batch: rx_ms[%zu] = %d (0 <= rx_ms < 604800000)", k, (int)rx_ms[k]);
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_dop_fix.grow(n_fix, e->stream)) return rc;
    if (int rc = e->d_dop_prior.grow(n_fix, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_obs, obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_rate_obs, rate_obs, n_obs)) return rc;
    if (int rc = upload(e, e->d_dop_rx_ms, rx_ms, n_fix)) return rc;
    if (int rc = doppler_fix_enqueue(e, eph, n_eph, e->d_nav_obs, e->d_rate_obs, e->d_dop_rx_ms, n_fix, sats_per_fix, fp, e->d_dop_fix,
                                     prior_out ? e->d_dop_prior.p : nullptr))
        return rc;
    if (int rc = download(e, fix_out, e->d_dop_fix, n_fix)) return rc;
    if (int rc = download(e, prior_out, e->d_dop_prior, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_cold_fix_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes, size_t stride,
                                      const void* d_tasks, const void* d_peaks, const void* d_rx_ms, size_t n_fix, int n_chans,
                                      const gpsacq_dopfine_params* dopfine_par, const gpsacq_doppler_fix_params* doppler_par,
                                      const gpsacq_refine_params* refine_par, const gpsacq_coarse_params* coarse_par, void* d_dopfine, void* d_rate_obs,
                                      void* d_doppler_fix, void* d_prior, void* d_fine, void* d_obs, void* d_fix, void* d_info, void* d_obs_out,
                                      int sync) {
    const char* who = "gpsacq_cold_fix";
    if (int rc = coarse_obs_check(who, e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_rx_ms || !d_info || !d_doppler_fix) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "%s: obs_out must not be obs", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    gpsacq_dopfine_params dp;
    gpsacq_doppler_fix_params fp;
    gpsacq_refine_params rp;
    gpsacq_coarse_params cp;
    if (int rc = refine_check(who, e, d_bits, n_bytes, stride, d_peaks, n_tasks, refine_par, d_fix, &rp)) return rc;
    if (int rc = dopfine_params(who, e, dopfine_par, &dp)) return rc;
    if (int rc = doppler_fix_params(who, doppler_par, &fp)) return rc;
    if (int rc = coarse_params(who, coarse_par, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_dopfine, e->d_dopfine, n_tasks)) return rc;
    if (int rc = or_own(e, d_rate_obs, e->d_rate_obs, n_tasks)) return rc;
    if (int rc = or_own(e, d_prior, e->d_dop_prior, n_fix)) return rc;
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = fine_dop_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, dp, d_dopfine)) return rc;
    if (int rc = coarse_obs_enqueue(e, d_peaks, n_fix, n_chans, dp.snr_min, d_obs)) return rc;
    if (int rc = rate_obs_fine_enqueue(e, d_peaks, d_dopfine, n_fix, n_chans, dp.snr_min, d_rate_obs)) return rc;
    if (int rc = doppler_fix_enqueue(e, eph, n_eph, d_obs, d_rate_obs, d_rx_ms, n_fix, n_chans, fp, d_doppler_fix, d_prior)) return rc;
    if (int rc = refine_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_doppler_last_ms(const gpsacq_engine* e, float* fine_dop_ms, float* rate_obs_ms, float* doppler_fix_ms) {
    if (!e || (!e->dop_fine_t.ran() && !e->dop_obs_t.ran() && !e->dop_fix_t.ran()))
        return fail(GPSACQ_ERR_ARG, "gpsacq_doppler_last_ms: no gpsacq_fine_doppler, gpsacq_rate_obs_fine or gpsacq_doppler_fix call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->dop_fine_t, fine_dop_ms)) return rc;
    if (int rc = stage_ms(e->dop_obs_t, rate_obs_ms)) return rc;
    return stage_ms(e->dop_fix_t, doppler_fix_ms);
}

// ---- snapshot chain on an 8-bit IQ capture (snapshot_iq_kernels.hip; sign mode: iq_kernels.hip, then the 1-bit kernels) ----------
namespace {
// a checked capture of this section and how its kernels reach it
struct IqSnap {
    bool sign = false;          // GPSACQ_SAMPLES_SIGN: the 1-bit kernels on the converted capture
    Capture cap;                // the conversion of sign mode
    const uint8_t* d_iq = nullptr;  // device
    size_t n_samples = 0, stride = 0;
    double mix_hz = 0.0, fc_lo = 0.0;  // multi-bit: f = lo_dop - mix_hz + fc_lo
    uint32_t flip = 0;
    int32_t dc_i = 0, dc_q = 0;
    const uint8_t* d_bits = nullptr;  // sign mode, after iq_snap_begin: the 1-bit stream in engine scratch
    size_t n_bytes = 0;
};
}  // namespace

// the arguments every form of this section shares; device: iq is a device pointer
static int iq_snap_check(const char* who, const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                         const void* peaks, size_t n_tasks, const void* out, bool device, IqSnap* s) {
    if (!e || !in || !iq || !peaks || !out || n_samples == 0 || n_tasks == 0 || n_tasks > 0x7fffffffu) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = iq8_capture(e, in, device ? iq : nullptr, stride, &s->cap)) return rc;
    if (stride % 16 != 0 || stride < 80000 || stride > ((size_t)1 << 31))
        return fail(GPSACQ_ERR_ARG, "%s: stride %zu (a multiple of 16 in 80000 .. 2^31)", who, stride);
    if (n_samples > ((size_t)1 << 55)) return fail(GPSACQ_ERR_ARG, "%s: n_samples %zu", who, n_samples);
    if (device && ((uintptr_t)iq & 15)) return fail(GPSACQ_ERR_ARG, "%s: IQ buffer must be 16-byte aligned", who);
    s->sign = in->multibit == GPSACQ_SAMPLES_SIGN;
    s->d_iq = device ? (const uint8_t*)iq : nullptr;
    s->n_samples = n_samples;
    s->stride = stride;
    if (!s->sign) {
        s->mix_hz = in->mix_hz;
        s->fc_lo = in->multibit == GPSACQ_SAMPLES_COMPLEX ? 0.0 : e->p.fc;
        s->flip = in->format == GPSACQ_IQ_U8 ? 0x80808080u : 0u;
        if (in->remove_dc) {
            if (!(std::fabs(in->mean_i) <= 128.5) || !(std::fabs(in->mean_q) <= 128.5))
                return fail(GPSACQ_ERR_ARG, "%s: mean (%g, %g) outside +-128", who, in->mean_i, in->mean_q);
            s->dc_i = (int32_t)std::nearbyint(in->mean_i);
            s->dc_q = (int32_t)std::nearbyint(in->mean_q);
            if (std::abs(s->dc_i) > 128 || std::abs(s->dc_q) > 128) return fail(GPSACQ_ERR_ARG, "%s: mean (%g, %g) outside +-128", who, in->mean_i, in->mean_q);
        }
    }
    return capture_engine_check(who, e);
}

// the host-buffer forms: the capture into engine scratch, and the tasks and the peaks where the caller gave some (the aided
// searches' peaks_in may be NULL)
static int iq_snap_upload(gpsacq_engine* e, IqSnap& s, const void* iq, const gpsacq_task* tasks, const gpsacq_peak* peaks, size_t n_tasks) {
    if (int rc = e->d_iq.grow(2 * s.n_samples + 16, e->stream)) return rc;
    HIPCHK(hipMemcpyAsync(e->d_iq, iq, 2 * s.n_samples, hipMemcpyHostToDevice, e->stream));
    s.d_iq = s.cap.d_src = e->d_iq;
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    if (peaks)
        if (int rc = upload(e, e->d_refine_peaks, peaks, n_tasks)) return rc;
    return GPSACQ_OK;
}

// sign mode converts the capture once per call, timed by `timer`, as gpsacq_track_iq8_device does
static int iq_snap_convert(gpsacq_engine* e, IqSnap& s, Stages<2>& timer) {
    s.n_bytes = (s.n_samples + 7) / 8;
    if (int rc = e->d_iqbits.grow(s.n_bytes, e->stream)) return rc;
    const size_t left = s.cap.iq_total > s.cap.iq_first ? s.cap.iq_total - s.cap.iq_first : 0;  // samples of the capture from iq[0] on
    if (int rc = timer.begin(e->stream)) return rc;
    if (left < s.n_samples) HIPCHK(hipMemsetAsync(e->d_iqbits, 0, s.n_bytes, e->stream));
    if (int rc = iq8_to_bits_enqueue(e, s.d_iq, std::min(s.n_samples, left), s.cap.iq, s.cap.iq_first, e->d_iqbits)) return rc;
    if (int rc = timer.mark(1, e->stream)) return rc;
    s.d_bits = e->d_iqbits;
    return timer.finish();
}

// a call of this section begins: no timer has run; sign mode converts the capture
static int iq_snap_begin(gpsacq_engine* e, IqSnap& s) {
    e->snapiq_conv_t.done = e->snapiq_refine_t.done = e->snapiq_dop_t.done = false;
    if (!s.sign) return GPSACQ_OK;
    return iq_snap_convert(e, s, e->snapiq_conv_t);
}

static void iq_capture_args(const gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_peaks, size_t n_tasks, IqCaptureArgs& c) {
    const bool ref_grid = e->sub == 1 && e->dstride == 1;  // as gpsacq_handoff_engine
    c.iq = s.d_iq;
    c.n_samples = s.n_samples;
    c.stride = s.stride;
    c.tasks = (const gpsacq_task*)d_tasks;
    c.peaks = (const gpsacq_peak*)d_peaks;
    c.n_tasks = n_tasks;
    c.chips = e->d_track_chips;
    c.fs = e->p.fs;
    c.step_hz = ref_grid ? 0.0 : e->p.fs / N_FFT * e->dstride / e->sub;
    c.mix_hz = s.mix_hz, c.fc_lo = s.fc_lo;
    c.spm = e->nlags;
    c.flip = s.flip;
    c.dc_i = s.dc_i, c.dc_q = s.dc_q;
}

// k_refine_iq, or k_refine on sign mode's stream, timed; every argument has been checked
static int refine_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_peaks, size_t n_tasks, const gpsacq_refine_params& rp,
                             void* d_fine) {
    if (int rc = ensure_track_chips(e)) return rc;
    return timed_stage(e->snapiq_refine_t, e->stream, [&] {
        if (s.sign) {
            RefineArgs a{};
            a.c = capture_args(e, s.d_bits, s.n_bytes, s.stride / 16, d_tasks, d_peaks, n_tasks);
            a.p = rp;
            a.out = (gpsacq_fine*)d_fine;
            launch_refine(a, e->stream);
        } else {
            RefineIqArgs a{};
            iq_capture_args(e, s, d_tasks, d_peaks, n_tasks, a.c);
            a.p = rp;
            a.out = (gpsacq_fine*)d_fine;
            launch_refine_iq(a, e->stream);
        }
    });
}

// k_fine_dop_iq, or k_fine_dop on sign mode's stream, timed; every argument has been checked
static int fine_dop_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_peaks, size_t n_tasks,
                               const gpsacq_dopfine_params& dp, void* d_dopfine) {
    if (int rc = ensure_track_chips(e)) return rc;
    return timed_stage(e->snapiq_dop_t, e->stream, [&] {
        if (s.sign) {
            FineDopArgs a{};
            a.c = capture_args(e, s.d_bits, s.n_bytes, s.stride / 16, d_tasks, d_peaks, n_tasks);
            a.p = dp;
            a.out = (gpsacq_dopfine*)d_dopfine;
            launch_fine_dop(a, e->stream);
        } else {
            FineDopIqArgs a{};
            iq_capture_args(e, s, d_tasks, d_peaks, n_tasks, a.c);
            a.p = dp;
            a.out = (gpsacq_dopfine*)d_dopfine;
            launch_fine_dop_iq(a, e->stream);
        }
    });
}

extern "C" int gpsacq_refine_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                        const void* d_tasks, const void* d_peaks, size_t n_tasks, const gpsacq_refine_params* params, void* d_fine,
                                        int sync) {
    IqSnap s;
    gpsacq_refine_params rp;
    if (int rc = iq_snap_check("gpsacq_refine_iq8", e, in, d_iq, n_samples, stride, d_peaks, n_tasks, d_fine, true, &s)) return rc;
    if (int rc = refine_params("gpsacq_refine_iq8", params, &rp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = refine_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_refine_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride, const gpsacq_task* tasks,
                                 const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_refine_params* params, gpsacq_fine* fine_out) {
    IqSnap s;
    gpsacq_refine_params rp;
    if (int rc = iq_snap_check("gpsacq_refine_iq8", e, in, iq, n_samples, stride, peaks, n_tasks, fine_out, false, &s)) return rc;
    if (int rc = refine_params("gpsacq_refine_iq8", params, &rp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_fine.grow(n_tasks, e->stream)) return rc;
    if (int rc = iq_snap_upload(e, s, iq, tasks, peaks, n_tasks)) return rc;
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = refine_iq_enqueue(e, s, tasks ? e->d_refine_tasks.p : nullptr, e->d_refine_peaks, n_tasks, rp, e->d_fine)) return rc;
    if (int rc = download(e, fine_out, e->d_fine, n_tasks)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fine_doppler_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_peaks, size_t n_tasks, const gpsacq_dopfine_params* params,
                                              void* d_dopfine, int sync) {
    IqSnap s;
    gpsacq_dopfine_params dp;
    if (int rc = iq_snap_check("gpsacq_fine_doppler_iq8", e, in, d_iq, n_samples, stride, d_peaks, n_tasks, d_dopfine, true, &s)) return rc;
    if (int rc = dopfine_params("gpsacq_fine_doppler_iq8", e, params, &dp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = fine_dop_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, dp, d_dopfine)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_fine_doppler_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_dopfine_params* params,
                                       gpsacq_dopfine* dopfine_out) {
    IqSnap s;
    gpsacq_dopfine_params dp;
    if (int rc = iq_snap_check("gpsacq_fine_doppler_iq8", e, in, iq, n_samples, stride, peaks, n_tasks, dopfine_out, false, &s)) return rc;
    if (int rc = dopfine_params("gpsacq_fine_doppler_iq8", e, params, &dp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_dopfine.grow(n_tasks, e->stream)) return rc;
    if (int rc = iq_snap_upload(e, s, iq, tasks, peaks, n_tasks)) return rc;
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = fine_dop_iq_enqueue(e, s, tasks ? e->d_refine_tasks.p : nullptr, e->d_refine_peaks, n_tasks, dp, e->d_dopfine)) return rc;
    if (int rc = download(e, dopfine_out, e->d_dopfine, n_tasks)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_fine_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                                 size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                 const gpsacq_refine_params* refine_par, const void* d_prior, const gpsacq_coarse_params* params,
                                                 void* d_fine, void* d_obs, void* d_fix, void* d_info, void* d_obs_out, int sync) {
    const char* who = "gpsacq_coarse_fix_fine_iq8";
    if (int rc = coarse_obs_check(who, e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_prior || !d_info) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "%s: obs_out must not be obs", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    IqSnap s;
    gpsacq_refine_params rp;
    gpsacq_coarse_params cp;
    if (int rc = iq_snap_check(who, e, in, d_iq, n_samples, stride, d_peaks, n_tasks, d_fix, true, &s)) return rc;
    if (int rc = refine_params(who, refine_par, &rp)) return rc;
    if (int rc = coarse_params(who, params, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = refine_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_cold_fix_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                          size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, const void* d_rx_ms, size_t n_fix,
                                          int n_chans, const gpsacq_dopfine_params* dopfine_par, const gpsacq_doppler_fix_params* doppler_par,
                                          const gpsacq_refine_params* refine_par, const gpsacq_coarse_params* coarse_par, void* d_dopfine,
                                          void* d_rate_obs, void* d_doppler_fix, void* d_prior, void* d_fine, void* d_obs, void* d_fix, void* d_info,
                                          void* d_obs_out, int sync) {
    const char* who = "gpsacq_cold_fix_iq8";
    if (int rc = coarse_obs_check(who, e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_rx_ms || !d_info || !d_doppler_fix) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "%s: obs_out must not be obs", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    IqSnap s;
    gpsacq_dopfine_params dp;
    gpsacq_doppler_fix_params fp;
    gpsacq_refine_params rp;
    gpsacq_coarse_params cp;
    if (int rc = iq_snap_check(who, e, in, d_iq, n_samples, stride, d_peaks, n_tasks, d_fix, true, &s)) return rc;
    if (int rc = refine_params(who, refine_par, &rp)) return rc;
    if (int rc = dopfine_params(who, e, dopfine_par, &dp)) return rc;
    if (int rc = doppler_fix_params(who, doppler_par, &fp)) return rc;
    if (int rc = coarse_params(who, coarse_par, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_dopfine, e->d_dopfine, n_tasks)) return rc;
    if (int rc = or_own(e, d_rate_obs, e->d_rate_obs, n_tasks)) return rc;
    if (int rc = or_own(e, d_prior, e->d_dop_prior, n_fix)) return rc;
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = iq_snap_begin(e, s)) return rc;
    if (int rc = fine_dop_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, dp, d_dopfine)) return rc;
    if (int rc = coarse_obs_enqueue(e, d_peaks, n_fix, n_chans, dp.snr_min, d_obs)) return rc;
    if (int rc = rate_obs_fine_enqueue(e, d_peaks, d_dopfine, n_fix, n_chans, dp.snr_min, d_rate_obs)) return rc;
    if (int rc = doppler_fix_enqueue(e, eph, n_eph, d_obs, d_rate_obs, d_rx_ms, n_fix, n_chans, fp, d_doppler_fix, d_prior)) return rc;
    if (int rc = refine_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snapshot_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* refine_ms, float* fine_dop_ms) {
    if (!e || (!e->snapiq_refine_t.ran() && !e->snapiq_dop_t.ran()))
        return fail(GPSACQ_ERR_ARG, "gpsacq_snapshot_iq8_last_ms: no gpsacq_refine_iq8, gpsacq_fine_doppler_iq8 or *_iq8_device chain on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->snapiq_conv_t, convert_ms)) return rc;
    if (int rc = stage_ms(e->snapiq_refine_t, refine_ms)) return rc;
    return stage_ms(e->snapiq_dop_t, fine_dop_ms);
}

// ---- aided acquisition: predicted code phase and Doppler, windowed search (aided_kernels.hip) ------------------------------------
extern "C" int gpsacq_aid_default_params(gpsacq_aid_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_aid_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->elev_min_deg = 5.0;
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_default_params(gpsacq_aided_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_aided_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->blocks = 16;
    p->min_segments = 1;
    p->code_half = 16;
    p->dop_half = 1;
    p->keep_snr = 25.0;    // the threshold of the search, as gpsacq_refine_default_params
    p->ratio_min = 1.922;  // the largest ratio of 2304 measured draws on absent PRNs (1.7376) plus a quarter of its excess over 1: include/gpsacq.h
    return GPSACQ_OK;
}

// the caller's parameters or the defaults into *out, checked
static int aid_params(const char* who, const gpsacq_aid_params* params, gpsacq_aid_params* out) {
    if (!params) return gpsacq_aid_default_params(out);
    *out = *params;
    if (!(out->elev_min_deg >= -90.0 && out->elev_min_deg <= 90.0))
        return fail(GPSACQ_ERR_ARG, "%s: elev_min_deg %g outside [-90, 90]", who, out->elev_min_deg);
    return GPSACQ_OK;
}

static int aided_params(const char* who, const gpsacq_aided_params* params, gpsacq_aided_params* out) {
    if (!params) return gpsacq_aided_default_params(out);
    *out = *params;
    if (out->blocks < 1 || out->blocks > 64) return fail(GPSACQ_ERR_ARG, "%s: blocks %d outside 1 .. 64", who, (int)out->blocks);
    if (out->min_segments < 1) return fail(GPSACQ_ERR_ARG, "%s: min_segments %d (must be >= 1)", who, (int)out->min_segments);
    if (out->code_half < 0 || out->code_half > AIDED_MAX_CODE_HALF)
        return fail(GPSACQ_ERR_ARG, "%s: code_half %d outside 0 .. %d", who, (int)out->code_half, AIDED_MAX_CODE_HALF);
    if (out->dop_half < 0 || out->dop_half > AIDED_MAX_DOP_HALF)
        return fail(GPSACQ_ERR_ARG, "%s: dop_half %d outside 0 .. %d", who, (int)out->dop_half, AIDED_MAX_DOP_HALF);
    if (!std::isfinite(out->keep_snr)) return fail(GPSACQ_ERR_ARG, "%s: keep_snr %g (must be finite)", who, out->keep_snr);
    if (!std::isfinite(out->ratio_min)) return fail(GPSACQ_ERR_ARG, "%s: ratio_min %g (must be finite)", who, out->ratio_min);
    return GPSACQ_OK;
}

// an engine the aided kernels serve: gpsacq_refine's, and coherent
static int aided_engine_check(const char* who, const gpsacq_engine* e) {
    if (e->nlags > 65535) return fail(GPSACQ_ERR_UNSUPPORTED, "%s: %d samples per millisecond (the packed counts hold 65535)", who, e->nlags);
    if (1.023e6 / e->p.fs + 1.0 / 1540.0 > REFINE_MAX_CHIPS_PER_SAMPLE)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: fs = %g Hz is fewer than %.2f samples per chip (a word's chips leave the kernel's window)", who, e->p.fs,
                    1.0 / REFINE_MAX_CHIPS_PER_SAMPLE);
    if (e->n_acc > 1) return fail(GPSACQ_ERR_UNSUPPORTED, "%s: the engine accumulates %d blocks (gpsacq_set_noncoherent)", who, e->n_acc);
    return GPSACQ_OK;
}

static int aid_predict_check(const char* who, const gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* fix, size_t n_fix, int n_chans,
                             const gpsacq_aid_params* params, const void* aid, gpsacq_aid_params* checked) {
    if (int rc = nav_check(who, e, eph, n_eph, fix, n_fix, aid)) return rc;
    if (n_chans < 1 || n_chans > GPSACQ_FIX_MAX_SATS) return fail(GPSACQ_ERR_ARG, "%s: n_chans %d outside 1 .. %d", who, n_chans, GPSACQ_FIX_MAX_SATS);
    if (int rc = aid_params(who, params, checked)) return rc;
    return aided_engine_check(who, e);
}

static int aided_check(const char* who, const gpsacq_engine* e, const void* bits, size_t n_bytes, size_t stride, const void* aid, const void* peaks_in,
                       size_t n_tasks, const gpsacq_aided_params* params, const void* aided, const void* peaks_out, gpsacq_aided_params* checked) {
    if (!aided || !peaks_out || (peaks_in && peaks_in == peaks_out)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = capture_check(who, e, bits, n_bytes, stride, aid, n_tasks, aided)) return rc;
    if (int rc = aided_params(who, params, checked)) return rc;
    return aided_engine_check(who, e);
}

// k_aid_predict, untimed; the ephemerides are up and every argument has been checked
static void aid_predict_launch(gpsacq_engine* e, int n_eph, const void* d_fix, const void* d_vel, size_t n_fix, int n_chans, const gpsacq_aid_params& ap,
                               void* d_aid) {
    AidPredictArgs a{};
    a.eph = e->d_nav_eph, a.n_eph = n_eph;
    a.fix = (const gpsacq_fix*)d_fix, a.vel = (const gpsacq_vel*)d_vel;
    a.n_fix = n_fix, a.chans = n_chans;
    a.fs = e->p.fs, a.step_hz = e->p.fs / N_FFT * e->dstride / e->sub;  // gpsacq_info.doppler_step_hz
    a.spm = e->nlags, a.kmax = e->kmax;
    a.p = ap;
    a.out = (gpsacq_aid*)d_aid;
    launch_aid_predict(a, e->stream);
}

// the ephemerides up, then k_aid_predict timed by `timer`; every argument has been checked
static int aid_predict_enqueue(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel, size_t n_fix, int n_chans,
                               const gpsacq_aid_params& ap, void* d_aid, Stages<2>& timer) {
    if (int rc = nav_upload_eph(e, eph, n_eph)) return rc;
    return timed_stage(timer, e->stream, [&] { aid_predict_launch(e, n_eph, d_fix, d_vel, n_fix, n_chans, ap, d_aid); });
}

// k_aided timed by `timer`; every argument has been checked
static int aided_enqueue(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_aid,
                         const void* d_peaks_in, size_t n_tasks, const gpsacq_aided_params& sp, void* d_aided, void* d_peaks_out, void* d_powers,
                         Stages<2>& timer) {
    if (int rc = ensure_track_chips(e)) return rc;
    AidedArgs a{};
    a.c = capture_args(e, d_bits, n_bytes, stride, d_tasks, d_peaks_in, n_tasks);
    a.kmax = e->kmax;
    a.aid = (const gpsacq_aid*)d_aid;
    a.p = sp;
    a.out = (gpsacq_aided*)d_aided;
    a.peaks_out = (gpsacq_peak*)d_peaks_out;
    a.powers = (unsigned long long*)d_powers;
    return timed_stage(timer, e->stream, [&] { launch_aided(a, e->stream); });
}

extern "C" int gpsacq_aid_predict_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel, size_t n_fix,
                                         int n_chans, const gpsacq_aid_params* params, void* d_aid, int sync) {
    gpsacq_aid_params ap;
    if (int rc = aid_predict_check("gpsacq_aid_predict", e, eph, n_eph, d_fix, n_fix, n_chans, params, d_aid, &ap)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = aid_predict_enqueue(e, eph, n_eph, d_fix, d_vel, n_fix, n_chans, ap, d_aid, e->aid_predict_t)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aid_predict(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_fix* fix, const gpsacq_vel* vel, size_t n_fix,
                                  int n_chans, const gpsacq_aid_params* params, gpsacq_aid* aid_out) {
    gpsacq_aid_params ap;
    if (int rc = aid_predict_check("gpsacq_aid_predict", e, eph, n_eph, fix, n_fix, n_chans, params, aid_out, &ap)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n = n_fix * (size_t)n_chans;
    if (int rc = e->d_aid.grow(n, e->stream)) return rc;
    if (int rc = upload(e, e->d_nav_fix, fix, n_fix)) return rc;
    if (vel)
        if (int rc = upload(e, e->d_vel, vel, n_fix)) return rc;
    if (int rc = aid_predict_enqueue(e, eph, n_eph, e->d_nav_fix, vel ? e->d_vel.p : nullptr, n_fix, n_chans, ap, e->d_aid, e->aid_predict_t)) return rc;
    if (int rc = download(e, aid_out, e->d_aid, n)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_search_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_aid,
                                          const void* d_peaks_in, size_t n_tasks, const gpsacq_aided_params* params, void* d_aided,
                                          void* d_peaks_out, void* d_powers_out, int sync) {
    gpsacq_aided_params sp;
    if (int rc = aided_check("gpsacq_aided_search", e, d_bits, n_bytes, stride, d_aid, d_peaks_in, n_tasks, params, d_aided, d_peaks_out, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = aided_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_aid, d_peaks_in, n_tasks, sp, d_aided, d_peaks_out, d_powers_out, e->aided_t)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_search(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks, const gpsacq_aid* aid,
                                   const gpsacq_peak* peaks_in, size_t n_tasks, const gpsacq_aided_params* params, gpsacq_aided* aided_out,
                                   gpsacq_peak* peaks_out, uint64_t* powers_out) {
    gpsacq_aided_params sp;
    if (int rc = aided_check("gpsacq_aided_search", e, bits, n_bytes, stride, aid, peaks_in, n_tasks, params, aided_out, peaks_out, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_pow = n_tasks * (size_t)(2 * sp.dop_half + 1) * (size_t)(2 * sp.code_half + 1);
    if (int rc = e->d_aided.grow(n_tasks, e->stream)) return rc;
    if (int rc = e->d_aided_peaks.grow(n_tasks, e->stream)) return rc;
    if (powers_out)
        if (int rc = e->d_aided_powers.grow(n_pow, e->stream)) return rc;
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    if (peaks_in)
        if (int rc = upload(e, e->d_refine_peaks, peaks_in, n_tasks)) return rc;
    if (int rc = upload(e, e->d_refine_bits, bits, n_bytes)) return rc;
    if (int rc = upload(e, e->d_aid, aid, n_tasks)) return rc;
    if (int rc = aided_enqueue(e, e->d_refine_bits, n_bytes, stride, tasks ? e->d_refine_tasks.p : nullptr, e->d_aid,
                               peaks_in ? e->d_refine_peaks.p : nullptr, n_tasks, sp, e->d_aided, e->d_aided_peaks,
                               powers_out ? e->d_aided_powers.p : nullptr, e->aided_t))
        return rc;
    if (int rc = download(e, aided_out, e->d_aided, n_tasks)) return rc;
    if (int rc = download(e, peaks_out, e->d_aided_peaks, n_tasks)) return rc;
    if (int rc = download(e, (unsigned long long*)powers_out, e->d_aided_powers, n_pow)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel,
                                         const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks_in, size_t n_fix,
                                         int n_chans, const gpsacq_aid_params* aid_par, const gpsacq_aided_params* aided_par, void* d_aid,
                                         void* d_aided, void* d_peaks_out, int sync) {
    const char* who = "gpsacq_aided_peaks";
    gpsacq_aid_params ap;
    gpsacq_aided_params sp;
    if (int rc = aid_predict_check(who, e, eph, n_eph, d_fix, n_fix, n_chans, aid_par, d_aided, &ap)) return rc;
    const size_t n_tasks = n_fix * (size_t)n_chans;
    if (int rc = aided_check(who, e, d_bits, n_bytes, stride, d_aided, d_peaks_in, n_tasks, aided_par, d_aided, d_peaks_out, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_aid, e->d_aid, n_tasks)) return rc;
    if (int rc = aid_predict_enqueue(e, eph, n_eph, d_fix, d_vel, n_fix, n_chans, ap, d_aid, e->aid_predict_t)) return rc;
    if (int rc = aided_enqueue(e, d_bits, n_bytes, stride, d_tasks, d_aid, d_peaks_in, n_tasks, sp, d_aided, d_peaks_out, nullptr, e->aided_t)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_last_ms(const gpsacq_engine* e, float* predict_ms, float* search_ms) {
    if (!e || (!e->aid_predict_t.ran() && !e->aided_t.ran()))
        return fail(GPSACQ_ERR_ARG, "gpsacq_aided_last_ms: no gpsacq_aid_predict or gpsacq_aided_search call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->aid_predict_t, predict_ms)) return rc;
    return stage_ms(e->aided_t, search_ms);
}

// ---- aided acquisition on an 8-bit IQ capture (aided_iq_kernels.hip; sign mode: iq_kernels.hip, then k_aided) ---------------------
extern "C" int gpsacq_aided_default_params_iq8(gpsacq_aided_params* p) {
    if (int rc = gpsacq_aided_default_params(p)) return rc;
    // the largest multi-bit ratio of 2304 measured draws on absent PRNs (2.9517) plus a quarter of its excess over 1: include/gpsacq.h
    p->ratio_min = 3.44;
    return GPSACQ_OK;
}

static int aided_iq_check(const char* who, const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                          const void* aid, const void* peaks_in, size_t n_tasks, const gpsacq_aided_params* params, const void* aided,
                          const void* peaks_out, bool device, IqSnap* s, gpsacq_aided_params* checked) {
    if (!aided || !peaks_out || (peaks_in && peaks_in == peaks_out)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = iq_snap_check(who, e, in, iq, n_samples, stride, aid, n_tasks, aided, device, s)) return rc;
    if (!params) {  // the defaults of the path that runs: sign mode is gpsacq_aided_search's, byte for byte
        if (int rc = s->sign ? gpsacq_aided_default_params(checked) : gpsacq_aided_default_params_iq8(checked)) return rc;
    } else if (int rc = aided_params(who, params, checked)) {
        return rc;
    }
    return aided_engine_check(who, e);
}

// a call of this section begins: no timer has run; sign mode converts the capture once
static int aided_iq_begin(gpsacq_engine* e, IqSnap& s) {
    e->aidiq_conv_t.done = e->aidiq_predict_t.done = e->aidiq_search_t.done = false;
    if (!s.sign) return GPSACQ_OK;
    return iq_snap_convert(e, s, e->aidiq_conv_t);
}

// k_aided_iq, or k_aided on sign mode's stream, timed; every argument has been checked
static int aided_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_aid, const void* d_peaks_in, size_t n_tasks,
                            const gpsacq_aided_params& sp, void* d_aided, void* d_peaks_out, void* d_powers) {
    if (s.sign) return aided_enqueue(e, s.d_bits, s.n_bytes, s.stride / 16, d_tasks, d_aid, d_peaks_in, n_tasks, sp, d_aided, d_peaks_out, d_powers, e->aidiq_search_t);
    if (int rc = ensure_track_chips(e)) return rc;
    AidedIqArgs a{};
    iq_capture_args(e, s, d_tasks, d_peaks_in, n_tasks, a.c);
    a.kmax = e->kmax;
    a.aid = (const gpsacq_aid*)d_aid;
    a.p = sp;
    a.out = (gpsacq_aided*)d_aided;
    a.peaks_out = (gpsacq_peak*)d_peaks_out;
    a.powers = (unsigned long long*)d_powers;
    return timed_stage(e->aidiq_search_t, e->stream, [&] { launch_aided_iq(a, e->stream); });
}

extern "C" int gpsacq_aided_search_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_aid, const void* d_peaks_in, size_t n_tasks,
                                              const gpsacq_aided_params* params, void* d_aided, void* d_peaks_out, void* d_powers_out, int sync) {
    IqSnap s;
    gpsacq_aided_params sp;
    if (int rc = aided_iq_check("gpsacq_aided_search_iq8", e, in, d_iq, n_samples, stride, d_aid, d_peaks_in, n_tasks, params, d_aided, d_peaks_out, true, &s,
                                &sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = aided_iq_begin(e, s)) return rc;
    if (int rc = aided_iq_enqueue(e, s, d_tasks, d_aid, d_peaks_in, n_tasks, sp, d_aided, d_peaks_out, d_powers_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_search_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_aid* aid, const gpsacq_peak* peaks_in, size_t n_tasks,
                                       const gpsacq_aided_params* params, gpsacq_aided* aided_out, gpsacq_peak* peaks_out, uint64_t* powers_out) {
    IqSnap s;
    gpsacq_aided_params sp;
    if (int rc = aided_iq_check("gpsacq_aided_search_iq8", e, in, iq, n_samples, stride, aid, peaks_in, n_tasks, params, aided_out, peaks_out, false, &s, &sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_pow = n_tasks * (size_t)(2 * sp.dop_half + 1) * (size_t)(2 * sp.code_half + 1);
    if (int rc = e->d_aided.grow(n_tasks, e->stream)) return rc;
    if (int rc = e->d_aided_peaks.grow(n_tasks, e->stream)) return rc;
    if (powers_out)
        if (int rc = e->d_aided_powers.grow(n_pow, e->stream)) return rc;
    if (int rc = iq_snap_upload(e, s, iq, tasks, peaks_in, n_tasks)) return rc;
    if (int rc = upload(e, e->d_aid, aid, n_tasks)) return rc;
    if (int rc = aided_iq_begin(e, s)) return rc;
    if (int rc = aided_iq_enqueue(e, s, tasks ? e->d_refine_tasks.p : nullptr, e->d_aid, peaks_in ? e->d_refine_peaks.p : nullptr, n_tasks, sp, e->d_aided,
                                  e->d_aided_peaks, powers_out ? e->d_aided_powers.p : nullptr))
        return rc;
    if (int rc = download(e, aided_out, e->d_aided, n_tasks)) return rc;
    if (int rc = download(e, peaks_out, e->d_aided_peaks, n_tasks)) return rc;
    if (int rc = download(e, (unsigned long long*)powers_out, e->d_aided_powers, n_pow)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_peaks_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel,
                                             const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride, const void* d_tasks,
                                             const void* d_peaks_in, size_t n_fix, int n_chans, const gpsacq_aid_params* aid_par,
                                             const gpsacq_aided_params* aided_par, void* d_aid, void* d_aided, void* d_peaks_out, int sync) {
    const char* who = "gpsacq_aided_peaks_iq8";
    gpsacq_aid_params ap;
    gpsacq_aided_params sp;
    IqSnap s;
    // d_aid may be NULL here (engine scratch), so the two checks are given d_aided where they test the prediction records for NULL
    if (int rc = aid_predict_check(who, e, eph, n_eph, d_fix, n_fix, n_chans, aid_par, d_aided, &ap)) return rc;
    const size_t n_tasks = n_fix * (size_t)n_chans;
    if (int rc = aided_iq_check(who, e, in, d_iq, n_samples, stride, d_aided, d_peaks_in, n_tasks, aided_par, d_aided, d_peaks_out, true, &s, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_aid, e->d_aid, n_tasks)) return rc;
    if (int rc = aided_iq_begin(e, s)) return rc;
    if (int rc = aid_predict_enqueue(e, eph, n_eph, d_fix, d_vel, n_fix, n_chans, ap, d_aid, e->aidiq_predict_t)) return rc;
    if (int rc = aided_iq_enqueue(e, s, d_tasks, d_aid, d_peaks_in, n_tasks, sp, d_aided, d_peaks_out, nullptr)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* predict_ms, float* search_ms) {
    if (!e || !e->aidiq_search_t.ran())
        return fail(GPSACQ_ERR_ARG, "gpsacq_aided_iq8_last_ms: no gpsacq_aided_search_iq8 or gpsacq_aided_peaks_iq8 call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->aidiq_conv_t, convert_ms)) return rc;
    if (int rc = stage_ms(e->aidiq_predict_t, predict_ms)) return rc;
    return stage_ms(e->aidiq_search_t, search_ms);
}

// ---- coherent aided acquisition: 20 ms sums, bit edge and fine Doppler (aided_kernels.hip) ----------------------------------------
extern "C" int gpsacq_aided_coh_table(int16_t* out) {
    if (!out) return fail(GPSACQ_ERR_ARG, "gpsacq_aided_coh_table: null argument");
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < COH_TABLE; ++k) {
        const double x = 2.0 * pi * (double)k / 1024.0;
        out[k] = (int16_t)std::nearbyint(16384.0 * std::cos(x));
        out[COH_TABLE + k] = (int16_t)std::nearbyint(16384.0 * std::sin(x));
    }
    return GPSACQ_OK;
}

// DEFAULT RATIO_MIN of "Coherent aided acquisition" (include/gpsacq.h): measured with tools/aided_floor.py --coherent
static constexpr double COH_RATIO_MIN = 10.73;  // the largest ratio of 2304 draws, 8.7837, plus a quarter of its excess over 1

extern "C" int gpsacq_aided_coh_default_params(gpsacq_aided_coh_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_aided_coh_default_params: null argument");
    std::memset(p, 0, sizeof *p);
    p->blocks = 16;
    p->min_segments = 20;
    p->code_half = 16;
    p->dop_half = 1;
    p->coh_ms = 20;
    p->fine_half = 3;
    p->fine_step = 25;  // 24.4 Hz at 5.456 MHz
    p->keep_snr = 25.0;
    p->ratio_min = COH_RATIO_MIN;  // the largest ratio of the measured draws on absent PRNs plus a quarter of its excess over 1: include/gpsacq.h
    return GPSACQ_OK;
}

static int aided_coh_params(const char* who, const gpsacq_engine* e, const gpsacq_aided_coh_params* params, gpsacq_aided_coh_params* out) {
    if (!params) {
        if (int rc = gpsacq_aided_coh_default_params(out)) return rc;
    } else {
        *out = *params;
    }
    const int M = out->coh_ms;
    if (out->blocks < 1 || out->blocks > 64) return fail(GPSACQ_ERR_ARG, "%s: blocks %d outside 1 .. 64", who, (int)out->blocks);
    if (out->min_segments < 1) return fail(GPSACQ_ERR_ARG, "%s: min_segments %d (must be >= 1)", who, (int)out->min_segments);
    if (out->code_half < 0 || out->code_half > COH_MAX_CODE_HALF)
        return fail(GPSACQ_ERR_ARG, "%s: code_half %d outside 0 .. %d", who, (int)out->code_half, COH_MAX_CODE_HALF);
    if (out->dop_half < 0 || out->dop_half > AIDED_MAX_DOP_HALF)
        return fail(GPSACQ_ERR_ARG, "%s: dop_half %d outside 0 .. %d", who, (int)out->dop_half, AIDED_MAX_DOP_HALF);
    if (M != 1 && M != 2 && M != 4 && M != 5 && M != 10 && M != 20) return fail(GPSACQ_ERR_ARG, "%s: coh_ms %d is none of 1, 2, 4, 5, 10, 20", who, M);
    if (out->fine_half < 0 || out->fine_half > COH_MAX_FINE_HALF)
        return fail(GPSACQ_ERR_ARG, "%s: fine_half %d outside 0 .. %d", who, (int)out->fine_half, COH_MAX_FINE_HALF);
    if (out->fine_step < 1 || out->fine_step > COH_MAX_FINE_STEP)
        return fail(GPSACQ_ERR_ARG, "%s: fine_step %d outside 1 .. %d", who, (int)out->fine_step, COH_MAX_FINE_STEP);
    if (!std::isfinite(out->keep_snr)) return fail(GPSACQ_ERR_ARG, "%s: keep_snr %g (must be finite)", who, out->keep_snr);
    if (!std::isfinite(out->ratio_min)) return fail(GPSACQ_ERR_ARG, "%s: ratio_min %g (must be finite)", who, out->ratio_min);
    if (!e) return GPSACQ_OK;
    if (int rc = aided_engine_check(who, e)) return rc;
    const long long fit = (long long)out->blocks * 40000 / e->nlags;
    if (fit * (2 * out->code_half + 1) > COH_MAX_Z)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: %lld segments of %d code phases (the z matrix holds %d entries)", who, fit, 2 * (int)out->code_half + 1,
                    COH_MAX_Z);
    if ((long long)M * 2 * e->nlags * ((long long)out->blocks * 40000) >= 1ll << 43)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: a power of %d ms sums could pass the key's 44 bits", who, M);
    return GPSACQ_OK;
}

static int aided_coh_check(const char* who, const gpsacq_engine* e, const void* bits, size_t n_bytes, size_t stride, const void* aid, const void* peaks_in,
                           size_t n_tasks, const gpsacq_aided_coh_params* params, const void* aided, const void* peaks_out,
                           gpsacq_aided_coh_params* checked) {
    if (!aided || !peaks_out || (peaks_in && peaks_in == peaks_out)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (!e) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (int rc = aided_coh_params(who, nullptr, params, checked)) return rc;  // the parameters' own ranges first: an argument error
    if (int rc = capture_check(who, e, bits, n_bytes, stride, aid, n_tasks, aided)) return rc;
    return aided_coh_params(who, e, params, checked);
}

static int ensure_coh_table(gpsacq_engine* e) {
    if (e->d_coh_table.p) return GPSACQ_OK;
    int16_t tab[2 * COH_TABLE];
    if (int rc = gpsacq_aided_coh_table(tab)) return rc;
    HIPCHK(e->d_coh_table.alloc(2 * COH_TABLE));
    HIPCHK(hipMemcpy(e->d_coh_table.p, tab, sizeof tab, hipMemcpyHostToDevice));
    return GPSACQ_OK;
}

static int instant_check(const char* who, const gpsacq_engine* e, const void* fix, const void* info, const void* prior, size_t n_fix, const void* out) {
    if (!e || !fix || !info || !prior || !out || n_fix == 0 || n_fix > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    return GPSACQ_OK;
}

// what a call of this section runs: any of the three stages, in this order, each timed; every argument has been checked
struct CohInstant {
    const void *d_fix, *d_info, *d_prior;
    size_t n_fix;
    void* d_out;
};
struct CohPredict {
    const gpsacq_ephemeris* eph;
    int n_eph;
    const void *d_fix, *d_vel;
    size_t n_fix;
    int n_chans;
    gpsacq_aid_params ap;
    void* d_aid;
};
struct CohSearch {
    const void* d_bits;
    size_t n_bytes, stride;
    const void *d_tasks, *d_aid, *d_peaks_in;
    size_t n_tasks;
    gpsacq_aided_coh_params sp;
    void *d_aided, *d_peaks_out, *d_powers;
};

// the chain's three stages on the engine's stream between the four events of `timer`; `ran` gets bit k for stage k + 1; `search`
// launches the search kernel, or is empty
template <class Search> static int coh_chain_enqueue(gpsacq_engine* e, Stages<4>& timer, int& ran, const CohInstant* in, const CohPredict* pr, bool has_search,
                                                     Search&& search) {
    if (pr)  // before the first event: the upload is no part of any stage's time
        if (int rc = nav_upload_eph(e, pr->eph, pr->n_eph)) return rc;
    ran = 0;
    if (int rc = timer.begin(e->stream)) return rc;
    if (in) {
        AidInstantArgs a{};
        a.fix = (const gpsacq_fix*)in->d_fix, a.info = (const gpsacq_coarse_info*)in->d_info, a.prior = (const gpsacq_coarse_prior*)in->d_prior;
        a.n_fix = in->n_fix;
        a.out = (gpsacq_fix*)in->d_out;
        launch_aid_instant(a, e->stream);
        ran |= 1;
    }
    if (int rc = timer.mark(1, e->stream)) return rc;
    if (pr) {
        aid_predict_launch(e, pr->n_eph, pr->d_fix, pr->d_vel, pr->n_fix, pr->n_chans, pr->ap, pr->d_aid);  // timed here alone: gpsacq_aided_last_ms keeps its own
        ran |= 2;
    }
    if (int rc = timer.mark(2, e->stream)) return rc;
    if (has_search) {
        search();
        ran |= 4;
    }
    if (int rc = timer.mark(3, e->stream)) return rc;
    return timer.finish();
}

// k_aided_coh on a 1-bit stream; every argument has been checked
static void aided_coh_launch(gpsacq_engine* e, const CohSearch& se) {
    AidedCohArgs a{};
    a.c = capture_args(e, se.d_bits, se.n_bytes, se.stride, se.d_tasks, se.d_peaks_in, se.n_tasks);
    a.kmax = e->kmax;
    a.aid = (const gpsacq_aid*)se.d_aid;
    a.table = e->d_coh_table;
    a.p = se.sp;
    a.out = (gpsacq_aided_coh*)se.d_aided;
    a.peaks_out = (gpsacq_peak*)se.d_peaks_out;
    a.powers = (unsigned long long*)se.d_powers;
    launch_aided_coh(a, e->stream);
}

static int aided_coh_enqueue(gpsacq_engine* e, const CohInstant* in, const CohPredict* pr, const CohSearch* se) {
    if (se) {
        if (int rc = ensure_track_chips(e)) return rc;
        if (int rc = ensure_coh_table(e)) return rc;
    }
    return coh_chain_enqueue(e, e->aided_coh_t, e->aided_coh_ran, in, pr, se != nullptr, [&] { aided_coh_launch(e, *se); });
}

static size_t coh_powers_per_task(const gpsacq_aided_coh_params& sp) {
    return (size_t)(2 * sp.dop_half + 1) * (size_t)(2 * sp.fine_half + 1) * (size_t)sp.coh_ms * (size_t)(2 * sp.code_half + 1);
}

extern "C" int gpsacq_aided_coh_search_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_aid,
                                              const void* d_peaks_in, size_t n_tasks, const gpsacq_aided_coh_params* params, void* d_aided,
                                              void* d_peaks_out, void* d_powers_out, int sync) {
    CohSearch se{d_bits, n_bytes, stride, d_tasks, d_aid, d_peaks_in, n_tasks, {}, d_aided, d_peaks_out, d_powers_out};
    if (int rc = aided_coh_check("gpsacq_aided_coh_search", e, d_bits, n_bytes, stride, d_aid, d_peaks_in, n_tasks, params, d_aided, d_peaks_out, &se.sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = aided_coh_enqueue(e, nullptr, nullptr, &se)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_search(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks, const gpsacq_aid* aid,
                                       const gpsacq_peak* peaks_in, size_t n_tasks, const gpsacq_aided_coh_params* params, gpsacq_aided_coh* aided_out,
                                       gpsacq_peak* peaks_out, uint64_t* powers_out) {
    gpsacq_aided_coh_params sp;
    if (int rc = aided_coh_check("gpsacq_aided_coh_search", e, bits, n_bytes, stride, aid, peaks_in, n_tasks, params, aided_out, peaks_out, &sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_pow = n_tasks * coh_powers_per_task(sp);
    if (int rc = e->d_aided_coh.grow(n_tasks, e->stream)) return rc;
    if (int rc = e->d_aided_peaks.grow(n_tasks, e->stream)) return rc;
    if (powers_out)
        if (int rc = e->d_coh_powers.grow(n_pow, e->stream)) return rc;
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    if (peaks_in)
        if (int rc = upload(e, e->d_refine_peaks, peaks_in, n_tasks)) return rc;
    if (int rc = upload(e, e->d_refine_bits, bits, n_bytes)) return rc;
    if (int rc = upload(e, e->d_aid, aid, n_tasks)) return rc;
    const CohSearch se{e->d_refine_bits, n_bytes, stride, tasks ? e->d_refine_tasks.p : nullptr, e->d_aid, peaks_in ? e->d_refine_peaks.p : nullptr, n_tasks, sp,
                       e->d_aided_coh, e->d_aided_peaks, powers_out ? e->d_coh_powers.p : nullptr};
    if (int rc = aided_coh_enqueue(e, nullptr, nullptr, &se)) return rc;
    if (int rc = download(e, aided_out, e->d_aided_coh, n_tasks)) return rc;
    if (int rc = download(e, peaks_out, e->d_aided_peaks, n_tasks)) return rc;
    if (int rc = download(e, (unsigned long long*)powers_out, e->d_coh_powers, n_pow)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aid_instant_device(gpsacq_engine* e, const void* d_fix, const void* d_info, const void* d_prior, size_t n_fix, void* d_fix_out,
                                         int sync) {
    if (int rc = instant_check("gpsacq_aid_instant", e, d_fix, d_info, d_prior, n_fix, d_fix_out)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const CohInstant in{d_fix, d_info, d_prior, n_fix, d_fix_out};
    if (int rc = aided_coh_enqueue(e, &in, nullptr, nullptr)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aid_instant(gpsacq_engine* e, const gpsacq_fix* fix, const gpsacq_coarse_info* coarse_info, const gpsacq_coarse_prior* prior,
                                  size_t n_fix, gpsacq_fix* fix_out) {
    if (int rc = instant_check("gpsacq_aid_instant", e, fix, coarse_info, prior, n_fix, fix_out)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = upload(e, e->d_nav_fix, fix, n_fix)) return rc;
    if (int rc = upload(e, e->d_coarse_info, coarse_info, n_fix)) return rc;
    if (int rc = upload(e, e->d_coarse_prior, prior, n_fix)) return rc;
    if (int rc = e->d_fix_instant.grow(n_fix, e->stream)) return rc;
    const CohInstant in{e->d_nav_fix, e->d_coarse_info, e->d_coarse_prior, n_fix, e->d_fix_instant};
    if (int rc = aided_coh_enqueue(e, &in, nullptr, nullptr)) return rc;
    if (int rc = download(e, fix_out, e->d_fix_instant, n_fix)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_info,
                                             const void* d_prior, const void* d_vel, const void* d_bits, size_t n_bytes, size_t stride,
                                             const void* d_tasks, const void* d_peaks_in, size_t n_fix, int n_chans, const gpsacq_aid_params* aid_par,
                                             const gpsacq_aided_coh_params* coh_par, void* d_fix_instant, void* d_aid, void* d_aided, void* d_peaks_out,
                                             int sync) {
    const char* who = "gpsacq_aided_coh_peaks";
    CohPredict pr{eph, n_eph, d_fix, d_vel, n_fix, n_chans, {}, nullptr};
    // d_aid may be NULL here (engine scratch), so the two checks below are given d_aided where they test the prediction records
    // for NULL: the chain's own required pointers are d_fix, d_bits, d_aided and d_peaks_out
    if (int rc = aid_predict_check(who, e, eph, n_eph, d_fix, n_fix, n_chans, aid_par, d_aided, &pr.ap)) return rc;
    if (d_info && !d_prior) return fail(GPSACQ_ERR_ARG, "%s: coarse-time records without their priors", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    CohSearch se{d_bits, n_bytes, stride, d_tasks, nullptr, d_peaks_in, n_tasks, {}, d_aided, d_peaks_out, nullptr};
    if (int rc = aided_coh_check(who, e, d_bits, n_bytes, stride, d_aided, d_peaks_in, n_tasks, coh_par, d_aided, d_peaks_out, &se.sp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_aid, e->d_aid, n_tasks)) return rc;
    CohInstant in{d_fix, d_info, d_prior, n_fix, d_fix_instant};
    if (d_info) {
        if (int rc = or_own(e, in.d_out, e->d_fix_instant, n_fix)) return rc;
        pr.d_fix = in.d_out;
    }
    pr.d_aid = d_aid, se.d_aid = d_aid;
    if (int rc = aided_coh_enqueue(e, d_info ? &in : nullptr, &pr, &se)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_last_ms(const gpsacq_engine* e, float* instant_ms, float* predict_ms, float* search_ms) {
    if (!e || !e->aided_coh_t.ran())
        return fail(GPSACQ_ERR_ARG, "gpsacq_aided_coh_last_ms: no gpsacq_aided_coh_search, gpsacq_aid_instant or gpsacq_aided_coh_peaks call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->aided_coh_t.wait()) return rc;
    float* const ms[3] = {instant_ms, predict_ms, search_ms};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        *ms[k] = 0.f;
        if (e->aided_coh_ran >> k & 1)
            if (int rc = e->aided_coh_t.elapsed(k, k + 1, ms[k])) return rc;
    }
    return GPSACQ_OK;
}

// ---- coherent aided acquisition on an 8-bit IQ capture (aided_coh_iq_kernels.hip; sign mode: iq_kernels.hip, then k_aided_coh) ------
// DEFAULT RATIO_MIN of "Coherent aided acquisition on an 8-bit IQ capture" (include/gpsacq.h): tools/aided_floor.py --iq8 --coherent
static constexpr double COH_IQ_RATIO_MIN = 28.56;  // the largest ratio of 2304 draws, 23.0511, plus a quarter of its excess over 1

extern "C" int gpsacq_aided_coh_default_params_iq8(gpsacq_aided_coh_params* p) {
    if (int rc = gpsacq_aided_coh_default_params(p)) return rc;
    p->ratio_min = COH_IQ_RATIO_MIN;  // the largest multi-bit ratio of the measured draws on absent PRNs plus a quarter of its excess over 1
    return GPSACQ_OK;
}

// what the multi-bit path refuses: gpsacq_aided_search's engines, the z matrix, and a power that could pass 63 bits (the header's
// BOUNDS: power <= M * (2^18 + 2^5) * spm * (blocks * 40000); the limits leave none)
static int aided_coh_iq_engine_check(const char* who, const gpsacq_engine* e, const gpsacq_aided_coh_params& sp) {
    if (int rc = aided_engine_check(who, e)) return rc;
    const long long fit = (long long)sp.blocks * 40000 / e->nlags;
    if (fit * (2 * sp.code_half + 1) > COH_MAX_Z)
        return fail(GPSACQ_ERR_UNSUPPORTED, "%s: %lld segments of %d code phases (the z matrix holds %d entries)", who, fit, 2 * (int)sp.code_half + 1, COH_MAX_Z);
    const unsigned __int128 bound = (unsigned __int128)sp.coh_ms * ((1u << 18) + (1u << 5)) * (unsigned)e->nlags * ((unsigned long long)sp.blocks * 40000ull);
    if (bound >= (unsigned __int128)1 << 63) return fail(GPSACQ_ERR_UNSUPPORTED, "%s: a power of %d ms sums could pass 63 bits", who, (int)sp.coh_ms);
    return GPSACQ_OK;
}

static int aided_coh_iq_check(const char* who, const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                              const void* aid, const void* peaks_in, size_t n_tasks, const gpsacq_aided_coh_params* params, const void* aided,
                              const void* peaks_out, bool device, IqSnap* s, gpsacq_aided_coh_params* checked) {
    if (!aided || !peaks_out || (peaks_in && peaks_in == peaks_out)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (!e) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (params)  // the parameters' own ranges first: an argument error
        if (int rc = aided_coh_params(who, nullptr, params, checked)) return rc;
    if (int rc = iq_snap_check(who, e, in, iq, n_samples, stride, aid, n_tasks, aided, device, s)) return rc;
    if (!params)  // the defaults of the path that runs: sign mode is gpsacq_aided_coh_search's, byte for byte
        if (int rc = s->sign ? gpsacq_aided_coh_default_params(checked) : gpsacq_aided_coh_default_params_iq8(checked)) return rc;
    if (s->sign) return aided_coh_params(who, e, checked, checked);
    return aided_coh_iq_engine_check(who, e, *checked);
}

// what the search stage of a call of this section runs; every argument has been checked
struct CohIqSearch {
    IqSnap s;
    const void *d_tasks, *d_aid, *d_peaks_in;
    size_t n_tasks;
    gpsacq_aided_coh_params sp;
    void *d_aided, *d_peaks_out, *d_powers;
};

// a call of this section: sign mode converts the capture once, then the chain's stages, each timed
static int aided_coh_iq_enqueue(gpsacq_engine* e, const CohInstant* in, const CohPredict* pr, CohIqSearch& se) {
    if (int rc = ensure_track_chips(e)) return rc;
    if (int rc = ensure_coh_table(e)) return rc;
    e->aidcohiq_conv_t.done = e->aidcohiq_t.done = false;
    if (se.s.sign)
        if (int rc = iq_snap_convert(e, se.s, e->aidcohiq_conv_t)) return rc;
    return coh_chain_enqueue(e, e->aidcohiq_t, e->aidcohiq_ran, in, pr, true, [&] {
        if (se.s.sign) {
            aided_coh_launch(e, CohSearch{se.s.d_bits, se.s.n_bytes, se.s.stride / 16, se.d_tasks, se.d_aid, se.d_peaks_in, se.n_tasks, se.sp, se.d_aided,
                                          se.d_peaks_out, se.d_powers});
            return;
        }
        AidedCohIqArgs a{};
        iq_capture_args(e, se.s, se.d_tasks, se.d_peaks_in, se.n_tasks, a.c);
        a.kmax = e->kmax;
        a.aid = (const gpsacq_aid*)se.d_aid;
        a.table = e->d_coh_table;
        a.p = se.sp;
        a.out = (gpsacq_aided_coh*)se.d_aided;
        a.peaks_out = (gpsacq_peak*)se.d_peaks_out;
        a.powers = (unsigned long long*)se.d_powers;
        launch_aided_coh_iq(a, e->stream);
    });
}

extern "C" int gpsacq_aided_coh_search_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                                  const void* d_tasks, const void* d_aid, const void* d_peaks_in, size_t n_tasks,
                                                  const gpsacq_aided_coh_params* params, void* d_aided, void* d_peaks_out, void* d_powers_out, int sync) {
    CohIqSearch se{{}, d_tasks, d_aid, d_peaks_in, n_tasks, {}, d_aided, d_peaks_out, d_powers_out};
    if (int rc = aided_coh_iq_check("gpsacq_aided_coh_search_iq8", e, in, d_iq, n_samples, stride, d_aid, d_peaks_in, n_tasks, params, d_aided, d_peaks_out, true,
                                    &se.s, &se.sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = aided_coh_iq_enqueue(e, nullptr, nullptr, se)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_search_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                           const gpsacq_task* tasks, const gpsacq_aid* aid, const gpsacq_peak* peaks_in, size_t n_tasks,
                                           const gpsacq_aided_coh_params* params, gpsacq_aided_coh* aided_out, gpsacq_peak* peaks_out,
                                           uint64_t* powers_out) {
    CohIqSearch se{};
    if (int rc = aided_coh_iq_check("gpsacq_aided_coh_search_iq8", e, in, iq, n_samples, stride, aid, peaks_in, n_tasks, params, aided_out, peaks_out, false,
                                    &se.s, &se.sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_pow = n_tasks * coh_powers_per_task(se.sp);
    if (int rc = e->d_aided_coh.grow(n_tasks, e->stream)) return rc;
    if (int rc = e->d_aided_peaks.grow(n_tasks, e->stream)) return rc;
    if (powers_out)
        if (int rc = e->d_coh_powers.grow(n_pow, e->stream)) return rc;
    if (int rc = iq_snap_upload(e, se.s, iq, tasks, peaks_in, n_tasks)) return rc;
    if (int rc = upload(e, e->d_aid, aid, n_tasks)) return rc;
    se.d_tasks = tasks ? e->d_refine_tasks.p : nullptr, se.d_aid = e->d_aid, se.d_peaks_in = peaks_in ? e->d_refine_peaks.p : nullptr;
    se.n_tasks = n_tasks;
    se.d_aided = e->d_aided_coh, se.d_peaks_out = e->d_aided_peaks, se.d_powers = powers_out ? e->d_coh_powers.p : nullptr;
    if (int rc = aided_coh_iq_enqueue(e, nullptr, nullptr, se)) return rc;
    if (int rc = download(e, aided_out, e->d_aided_coh, n_tasks)) return rc;
    if (int rc = download(e, peaks_out, e->d_aided_peaks, n_tasks)) return rc;
    if (int rc = download(e, (unsigned long long*)powers_out, e->d_coh_powers, n_pow)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_peaks_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_info,
                                                 const void* d_prior, const void* d_vel, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples,
                                                 size_t stride, const void* d_tasks, const void* d_peaks_in, size_t n_fix, int n_chans,
                                                 const gpsacq_aid_params* aid_par, const gpsacq_aided_coh_params* coh_par, void* d_fix_instant, void* d_aid,
                                                 void* d_aided, void* d_peaks_out, int sync) {
    const char* who = "gpsacq_aided_coh_peaks_iq8";
    CohPredict pr{eph, n_eph, d_fix, d_vel, n_fix, n_chans, {}, nullptr};
    // d_aid may be NULL here (engine scratch), so the two checks are given d_aided where they test the prediction records for NULL
    if (int rc = aid_predict_check(who, e, eph, n_eph, d_fix, n_fix, n_chans, aid_par, d_aided, &pr.ap)) return rc;
    if (d_info && !d_prior) return fail(GPSACQ_ERR_ARG, "%s: coarse-time records without their priors", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    CohIqSearch se{{}, d_tasks, nullptr, d_peaks_in, n_tasks, {}, d_aided, d_peaks_out, nullptr};
    if (int rc = aided_coh_iq_check(who, e, in, d_iq, n_samples, stride, d_aided, d_peaks_in, n_tasks, coh_par, d_aided, d_peaks_out, true, &se.s, &se.sp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_aid, e->d_aid, n_tasks)) return rc;
    CohInstant ins{d_fix, d_info, d_prior, n_fix, d_fix_instant};
    if (d_info) {
        if (int rc = or_own(e, ins.d_out, e->d_fix_instant, n_fix)) return rc;
        pr.d_fix = ins.d_out;
    }
    pr.d_aid = d_aid, se.d_aid = d_aid;
    if (int rc = aided_coh_iq_enqueue(e, d_info ? &ins : nullptr, &pr, se)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_aided_coh_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* instant_ms, float* predict_ms, float* search_ms) {
    if (!e || !e->aidcohiq_t.ran())
        return fail(GPSACQ_ERR_ARG, "gpsacq_aided_coh_iq8_last_ms: no gpsacq_aided_coh_search_iq8 or gpsacq_aided_coh_peaks_iq8 call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->aidcohiq_conv_t, convert_ms)) return rc;
    if (int rc = e->aidcohiq_t.wait()) return rc;
    float* const ms[3] = {instant_ms, predict_ms, search_ms};
    for (int k = 0; k < 3; ++k) {
        if (!ms[k]) continue;
        *ms[k] = 0.f;
        if (e->aidcohiq_ran >> k & 1)
            if (int rc = e->aidcohiq_t.elapsed(k, k + 1, ms[k])) return rc;
    }
    return GPSACQ_OK;
}

// ---- snapshot signal quality on an 8-bit IQ capture (snapq_iq_kernels.hip; sign mode: snapq_kernels.hip) ---------------------------
static constexpr double SNAPQ_IQ_CN0_MIN_LIN = 1432.4;  // the largest lin of 2304 absent draws, 1145.93 Hz, plus a quarter of it

extern "C" int gpsacq_snap_quality_default_params_iq8(gpsacq_snap_quality_params* p) {
    if (!p) return fail(GPSACQ_ERR_ARG, "gpsacq_snap_quality_default_params_iq8: null argument");
    std::memset(p, 0, sizeof *p);
    p->min_segments = 1;
    p->cn0_min_lin = SNAPQ_IQ_CN0_MIN_LIN;
    p->cn0_ref_lin = std::pow(10.0, 4.86);  // 48.6 dB-Hz: what the amplitude-0.2 satellites of the bench scene read
    return GPSACQ_OK;
}

// the caller's parameters, or the defaults of the capture's mode, into *out, checked
static int snap_quality_iq_params(const char* who, const IqSnap& s, const gpsacq_snap_quality_params* params, gpsacq_snap_quality_params* out) {
    if (!params && !s.sign) return gpsacq_snap_quality_default_params_iq8(out);
    return snap_quality_params(who, params, out);
}

static int snap_quality_iq_check(const char* who, const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                 const void* fine, size_t n_fix, int n_chans, const gpsacq_snap_quality_params* params, const void* info, bool device,
                                 IqSnap* s, gpsacq_snap_quality_params* checked) {
    if (n_fix > ((size_t)1 << 31)) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (n_chans < 1 || n_chans > GPSACQ_FIX_MAX_SATS) return fail(GPSACQ_ERR_ARG, "%s: n_chans %d outside 1 .. %d", who, n_chans, GPSACQ_FIX_MAX_SATS);
    if (int rc = iq_snap_check(who, e, in, iq, n_samples, stride, fine, n_fix * (size_t)n_chans, info, device, s)) return rc;
    return snap_quality_iq_params(who, *s, params, checked);
}

static SnapIqCapture snap_iq_capture(const IqSnap& s) { return SnapIqCapture{s.d_iq, s.n_samples, s.flip, s.dc_i, s.dc_q}; }

static SnapWindowArgs snap_window_args(const gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_fine, size_t n_tasks) {
    return SnapWindowArgs{(const gpsacq_task*)d_tasks, (const gpsacq_fine*)d_fine, n_tasks, s.n_samples, s.stride, e->nlags};
}

// a call of this section begins: no timer has run
static void snap_quality_iq_begin(gpsacq_engine* e) { e->snapqiq_floor_t.done = e->snapqiq_quality_t.done = false; }

// k_iq_energy over the capture's whole chunks and k_snap_floor (sign mode: k_snap_floor alone), timed; every argument has been checked
static int snap_floor_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_fine, size_t n_tasks, void* d_floor) {
    const size_t n_chunks = s.sign ? 0 : s.n_samples / SNAPQ_CHUNK;
    if (int rc = e->d_chunk_energy.grow(n_chunks, e->stream)) return rc;
    if (int rc = e->snapqiq_floor_t.begin(e->stream)) return rc;
    if (!s.sign) launch_iq_energy(IqEnergyArgs{snap_iq_capture(s), n_chunks, e->d_chunk_energy}, e->stream);
    launch_snap_floor(SnapFloorArgs{snap_iq_capture(s), snap_window_args(e, s, d_tasks, d_fine, n_tasks), e->d_chunk_energy, n_chunks, s.sign ? 1 : 0,
                                    (uint64_t*)d_floor},
                      e->stream);
    if (int rc = e->snapqiq_floor_t.mark(1, e->stream)) return rc;
    return e->snapqiq_floor_t.finish();
}

// k_snap_quality_iq on k_snap_floor's floors, or k_snap_quality in sign mode, timed; every argument has been checked
static int snap_quality_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_fine, size_t n_fix, int n_chans,
                                   const gpsacq_snap_quality_params& qp, void* d_obs, const void* d_floor, void* d_info) {
    const size_t n_tasks = n_fix * (size_t)n_chans;
    return timed_stage(e->snapqiq_quality_t, e->stream, [&] {
        if (s.sign)
            launch_snap_quality(SnapQualityArgs{(const gpsacq_fine*)d_fine, n_tasks, e->nlags, e->p.fs, qp, (gpsacq_obs*)d_obs, (gpsacq_quality_info*)d_info},
                                e->stream);
        else
            launch_snap_quality_iq(SnapQualityIqArgs{snap_window_args(e, s, d_tasks, d_fine, n_tasks), (const uint64_t*)d_floor, e->p.fs, qp, (gpsacq_obs*)d_obs,
                                                     (gpsacq_quality_info*)d_info},
                                   e->stream);
    });
}

// floors, then quality: in sign mode the floors are written only where the caller asked for them
static int snap_floor_quality_iq_enqueue(gpsacq_engine* e, const IqSnap& s, const void* d_tasks, const void* d_fine, size_t n_fix, int n_chans,
                                         const gpsacq_snap_quality_params& qp, void* d_obs, void* d_floor, void* d_info) {
    const size_t n_tasks = n_fix * (size_t)n_chans;
    if (!s.sign || d_floor) {
        if (int rc = or_own(e, d_floor, e->d_snap_floor, n_tasks)) return rc;
        if (int rc = snap_floor_iq_enqueue(e, s, d_tasks, d_fine, n_tasks, d_floor)) return rc;
    }
    return snap_quality_iq_enqueue(e, s, d_tasks, d_fine, n_fix, n_chans, qp, d_obs, d_floor, d_info);
}

// the host-buffer forms: the capture (multi-bit mode only: sign mode does not read it), the tasks and the records into engine scratch
static int snap_quality_iq_upload(gpsacq_engine* e, IqSnap& s, const void* iq, const gpsacq_task* tasks, const gpsacq_fine* fine, size_t n_tasks) {
    if (!s.sign) {
        if (int rc = e->d_iq.grow(2 * s.n_samples + 16, e->stream)) return rc;
        HIPCHK(hipMemcpyAsync(e->d_iq, iq, 2 * s.n_samples, hipMemcpyHostToDevice, e->stream));
        s.d_iq = e->d_iq;
    }
    if (tasks)
        if (int rc = upload(e, e->d_refine_tasks, tasks, n_tasks)) return rc;
    return upload(e, e->d_fine, fine, n_tasks);
}

extern "C" int gpsacq_snap_floor_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                            const void* d_tasks, const void* d_fine, size_t n_tasks, void* d_floor, int sync) {
    IqSnap s;
    if (int rc = iq_snap_check("gpsacq_snap_floor_iq8", e, in, d_iq, n_samples, stride, d_fine, n_tasks, d_floor, true, &s)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    snap_quality_iq_begin(e);
    if (int rc = snap_floor_iq_enqueue(e, s, d_tasks, d_fine, n_tasks, d_floor)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_floor_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride, const gpsacq_task* tasks,
                                     const gpsacq_fine* fine, size_t n_tasks, uint64_t* floor_out) {
    IqSnap s;
    if (int rc = iq_snap_check("gpsacq_snap_floor_iq8", e, in, iq, n_samples, stride, fine, n_tasks, floor_out, false, &s)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = e->d_snap_floor.grow(n_tasks, e->stream)) return rc;
    if (int rc = snap_quality_iq_upload(e, s, iq, tasks, fine, n_tasks)) return rc;
    snap_quality_iq_begin(e);
    if (int rc = snap_floor_iq_enqueue(e, s, tasks ? e->d_refine_tasks.p : nullptr, e->d_fine, n_tasks, e->d_snap_floor)) return rc;
    if (int rc = download(e, floor_out, e->d_snap_floor, n_tasks)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_quality_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_fine, size_t n_fix, int n_chans,
                                              const gpsacq_snap_quality_params* params, void* d_obs, void* d_floor, void* d_info, int sync) {
    IqSnap s;
    gpsacq_snap_quality_params qp;
    if (int rc = snap_quality_iq_check("gpsacq_snap_quality_iq8", e, in, d_iq, n_samples, stride, d_fine, n_fix, n_chans, params, d_info, true, &s, &qp))
        return rc;
    HIPCHK(hipSetDevice(e->p.device));
    snap_quality_iq_begin(e);
    if (int rc = snap_floor_quality_iq_enqueue(e, s, d_tasks, d_fine, n_fix, n_chans, qp, d_obs, d_floor, d_info)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_quality_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_fine* fine, size_t n_fix, int n_chans,
                                       const gpsacq_snap_quality_params* params, gpsacq_obs* obs, gpsacq_quality_info* info) {
    IqSnap s;
    gpsacq_snap_quality_params qp;
    if (int rc = snap_quality_iq_check("gpsacq_snap_quality_iq8", e, in, iq, n_samples, stride, fine, n_fix, n_chans, params, info, false, &s, &qp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    const size_t n_obs = n_fix * (size_t)n_chans;
    if (int rc = e->d_snapq_info.grow(n_obs, e->stream)) return rc;
    if (int rc = snap_quality_iq_upload(e, s, iq, tasks, fine, n_obs)) return rc;
    if (obs)
        if (int rc = upload(e, e->d_coarse_obs, (const gpsacq_obs*)obs, n_obs)) return rc;
    snap_quality_iq_begin(e);
    if (int rc = snap_floor_quality_iq_enqueue(e, s, tasks ? e->d_refine_tasks.p : nullptr, e->d_fine, n_fix, n_chans, qp, obs ? e->d_coarse_obs.p : nullptr,
                                               nullptr, e->d_snapq_info))
        return rc;
    if (int rc = download(e, obs, e->d_coarse_obs, n_obs)) return rc;
    if (int rc = download(e, info, e->d_snapq_info, n_obs)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_coarse_fix_quality_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                                    size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                    const gpsacq_refine_params* refine_par, const gpsacq_snap_quality_params* quality_par,
                                                    const void* d_prior, const gpsacq_coarse_params* params, void* d_fine, void* d_obs, void* d_floor,
                                                    void* d_qinfo, void* d_fix, void* d_info, void* d_obs_out, int sync) {
    const char* who = "gpsacq_coarse_fix_quality_iq8";
    if (int rc = coarse_obs_check(who, e, d_peaks, n_fix, n_chans, 0.0, d_fix)) return rc;
    if (!eph || n_eph <= 0 || !d_prior || !d_info) return fail(GPSACQ_ERR_ARG, "%s: bad argument", who);
    if (d_obs && d_obs_out == d_obs) return fail(GPSACQ_ERR_ARG, "%s: obs_out must not be obs", who);
    const size_t n_tasks = n_fix * (size_t)n_chans;
    IqSnap s;
    gpsacq_refine_params rp;
    gpsacq_snap_quality_params qp;
    gpsacq_coarse_params cp;
    if (int rc = iq_snap_check(who, e, in, d_iq, n_samples, stride, d_peaks, n_tasks, d_fix, true, &s)) return rc;
    if (int rc = refine_params(who, refine_par, &rp)) return rc;
    if (int rc = snap_quality_iq_params(who, s, quality_par, &qp)) return rc;
    if (int rc = coarse_params(who, params, &cp)) return rc;
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = or_own(e, d_fine, e->d_fine, n_tasks)) return rc;
    if (int rc = or_own(e, d_obs, e->d_coarse_obs, n_tasks)) return rc;
    if (int rc = or_own(e, d_qinfo, e->d_snapq_info, n_tasks)) return rc;
    if (int rc = iq_snap_begin(e, s)) return rc;
    snap_quality_iq_begin(e);
    if (int rc = refine_iq_enqueue(e, s, d_tasks, d_peaks, n_tasks, rp, d_fine)) return rc;
    if (int rc = coarse_obs_fine_enqueue(e, d_peaks, d_fine, n_fix, n_chans, rp.snr_min, d_obs)) return rc;
    if (int rc = snap_floor_quality_iq_enqueue(e, s, d_tasks, d_fine, n_fix, n_chans, qp, d_obs, d_floor, d_qinfo)) return rc;
    if (int rc = coarse_fix_enqueue(e, eph, n_eph, d_obs, d_prior, n_fix, n_chans, cp, d_fix, d_info, d_obs_out)) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return GPSACQ_OK;
}

extern "C" int gpsacq_snap_quality_iq8_last_ms(const gpsacq_engine* e, float* floor_ms, float* quality_ms) {
    if (!e || (!e->snapqiq_floor_t.ran() && !e->snapqiq_quality_t.ran()))
        return fail(GPSACQ_ERR_ARG, "gpsacq_snap_quality_iq8_last_ms: no gpsacq_snap_floor_iq8, gpsacq_snap_quality_iq8 or gpsacq_coarse_fix_quality_iq8 call on this engine");
    HIPCHK(hipSetDevice(e->p.device));
    if (int rc = stage_ms(e->snapqiq_floor_t, floor_ms)) return rc;
    return stage_ms(e->snapqiq_quality_t, quality_ms);
}
