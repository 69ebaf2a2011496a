// nav_launch.hpp -- argument blocks and launchers of the navigation solver of include/gpsacq.h ("Navigation solver"):
// nav_kernels.hip's k_sat_state (one lane per observation) and k_fix (one lane per fix), and of "Velocity and clock drift":
// k_sat_state_rate (one lane per observation) and k_vel (one lane per fix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

constexpr int NAV_BLOCK = 64;  // lanes per workgroup of both kernels: one wave, so a short batch still spreads over the CUs

// one ephemeris as the kernels read it: gpsacq_ephemeris's orbit and clock terms, the reference epochs in milliseconds, and the
// verdict of gpsacq_ephemeris_valid()
struct NavEph {
    double t_gd, a_f0, a_f1, a_f2;
    double c_rs, dn, m_0, c_uc, e, c_us, sqrt_a;
    double c_ic, omega_0, c_is, i_0, c_rc, omega, omega_dot, idot;
    int32_t toc_ms, toe_ms;
    int32_t valid, reserved;
};  // 168 bytes

struct SatStateArgs {
    const NavEph* eph;  // [n_eph] (device)
    int n_eph;
    const gpsacq_obs* obs;  // [n_obs] (device)
    size_t n_obs;
    gpsacq_sat_state* out;  // [n_obs] (device)
};
void launch_sat_state(const SatStateArgs& a, hipStream_t s);

struct FixArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;          // [n_fix][sats] (device)
    const gpsacq_sat_state* state;  // [n_fix][sats], k_sat_state's output for obs
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_fix* out;  // [n_fix] (device)
};
void launch_fix(const FixArgs& a, hipStream_t s);

struct SatRateArgs {
    const NavEph* eph;  // [n_eph] (device)
    int n_eph;
    const gpsacq_obs* obs;  // [n_obs] (device)
    size_t n_obs;
    gpsacq_sat_rate* out;  // [n_obs] (device)
};
void launch_sat_state_rate(const SatRateArgs& a, hipStream_t s);

struct VelArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;            // [n_fix][sats] (device)
    const gpsacq_rate_obs* rate_obs;  // [n_fix][sats]
    const gpsacq_sat_state* state;    // [n_fix][sats], k_sat_state's output for obs
    const gpsacq_sat_rate* rate;      // [n_fix][sats], k_sat_state_rate's output for obs
    const gpsacq_fix* fix;            // [n_fix]
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_vel* out;  // [n_fix] (device)
};
void launch_vel(const VelArgs& a, hipStream_t s);

}  // namespace acq
