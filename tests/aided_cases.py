"""The scene of the aided-acquisition tests (tests/test_aided.py on the CPU, tests/test_gpu_aided.py on the GPU): the northern
receiver's best eight satellites, of which five are in the capture at amplitude 0.2, one at WEAK_AMPLITUDE and two are ABSENT --
with a prediction as good as the others', but no signal.  Also a plain numpy FFT search of one block, to show what the unaided
search makes of the weak one."""
import numpy as np

import track_ref
from coarse_helpers import synth_sats
from nav_helpers import geometry

FS, FC, SPM, BLOCK_BYTES = 5.456e6, 4.092e6, 5456, 5120
KMAX = 36          # the reference grid: +-5 kHz in bins of fs / 40000
STEP_HZ = FS / 40000
L1, CPS = 1575.42e6, 1.023e6
# chosen on the CPU by tests/test_aided.py::test_detection_of_a_weak_satellite, whose docstring has the three figures
WEAK_AMPLITUDE = 0.05
REF_FRAC = 0.6180e-3  # the receive time of the capture's first sample is (geo["ref_ms"] + 4321, REF_FRAC)


def scene_sats(weak=WEAK_AMPLITUDE, first_sample=0):
    """(geo, sel, sats in the capture (five strong, then the weak one), the two absent satellites as gpsacq_sat tuples of amplitude
    0, the Dopplers of all eight).  Column c of sel is channel c everywhere"""
    geo = geometry("north")
    sel = geo["subsets"][8]
    sats, dops = synth_sats(geo, sel, geo["ref_ms"] + 4321, REF_FRAC, first_sample, FS, 0.2)
    present = [s for s in sats[:5]] + [(sats[5][0], weak) + tuple(sats[5][2:])]
    absent = [(s[0], 0.0) + tuple(s[2:]) for s in sats[6:]]
    return geo, sel, present, absent, dops


def law_center(sat, m0):
    """(ca_shift, lo_shift) the generator's law gives satellite `sat` at sample m0: the code position (m0 + code_phase) *
    chips_per_sample there, in samples of the nominal code rate as FROM PEAKS reads it, and the Doppler in grid steps -- floats"""
    cps = CPS * (1.0 + sat[2] / L1) / FS
    return ((m0 + sat[3]) * cps % 1023.0) / CPS * FS, sat[2] / STEP_HZ


def numpy_search(samples01, prn):
    """the search's figure for one block of 40000 samples (0/1): per Doppler bin of fs / 40000 within +-KMAX the circular
    correlation of the carrier-wiped samples with the code sampled at fs, by FFT; snr = the largest power over the lags 0 .. spm - 1
    and all bins / the mean power of that bin's lags.  Returns (snr, lo_shift, ca_shift)"""
    n = 40000
    m = np.arange(n)
    x = 1.0 - 2.0 * samples01[:n].astype(np.float64)
    code = 1.0 - 2.0 * track_ref.chips(prn)[np.floor(m * (CPS / FS)).astype(np.int64) % 1023]
    cf = np.conj(np.fft.fft(code))
    best = (0.0, 0, 0)
    for d in range(-KMAX, KMAX + 1):
        z = x * np.exp(-2j * np.pi * (((FC + d * STEP_HZ) / FS * m) % 1.0))
        p = np.abs(np.fft.ifft(np.fft.fft(z) * cf)[:SPM]) ** 2
        snr = float(p.max() / p.mean())
        if snr > best[0]:
            best = (snr, d, int((SPM - p.argmax()) % SPM))
    return best
