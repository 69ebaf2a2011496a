"""What the aided-acquisition tests on an 8-bit IQ capture share (tests/test_aided_iq.py on the CPU, tests/test_gpu_aided_iq.py on
the GPU): the rate, the eight sample modes, the predictions that reach the edges and the weak scene."""
import numpy as np

FS, FC, SPM = 5.456e6, 4.092e6, 5456
KMAX = 36          # the reference grid: +-5 kHz in bins of fs / 40000
STEP_HZ = FS / 40000
L1, CPS = 1575.42e6, 1.023e6
REAL, COMPLEX = 1, 2
MEAN = (3.4, -2.6)
# (signed, remove_dc, multibit): format x mean x REAL / COMPLEX
MODES = [(signed, dc, mb) for signed in (True, False) for dc in (False, True) for mb in (REAL, COMPLEX)]

# The gain scene: five satellites at 0.2 and a weak one whose Dopplers lie evenly over the +-5 kHz of the search, 1600 Hz apart (two
# satellites near zero Doppler share this rate's staircase error: tests/test_snapshot_iq.py), two ABSENT PRNs with a prediction and no
# signal.  IF 0.4 MHz, scale 16, sigma 1, int8, as tools/snapshot_bench.py --iq8.
IF_HZ, SCALE = 0.4e6, 16.0
STRONG = [(3, 0.2, -4100.0, 100.3, 0.1), (11, 0.2, -2500.0, 4000.7, 0.4), (17, 0.2, -900.0, 2727.45, 0.7), (22, 0.2, 900.0, 1801.2, 0.25),
          (28, 0.2, 2500.0, 5120.6, 0.9)]
WEAK_SAT = (32, None, 4100.0, 777.77, 0.55)
ABSENT = [(7, 0.0, -1700.0, 3111.1, 0.0), (25, 0.0, 3300.0, 1999.9, 0.0)]
# chosen on the CPU by tests/test_aided_iq.py::test_the_gain_over_the_sign_path, whose docstring has the figures: on the header's
# WHAT TO EXPECT ladder of "Aided acquisition" (0.03 .. 0.05), where the sign path reads 1.98 against its ratio_min of 1.922
WEAK_AMPLITUDE = 0.04


def mix_of(multibit, if_hz, fc=FC):
    """the mix_hz with which a search of the capture reports lo_shift = round(doppler * 40000 / fs)"""
    return -if_hz if multibit == COMPLEX else fc - if_hz


def as_u8(iq):
    return (np.asarray(iq).view(np.int8).astype(np.int16) + 128).astype(np.uint8)


def ref_kw(signed, dc, multibit, if_hz, fc=FC):
    return dict(signed=signed, mean=MEAN if dc else None, mix_hz=mix_of(multibit, if_hz, fc), multibit=multibit)


def hand_aid(dtype, kmax, spm, step_hz, n, seed, max_block=1):
    """n hand-made predictions that reach the edges: ca_center in {0, 1, spm / 2, spm - 1} (base + h crosses spm on both sides) x
    lo_center in {-kmax, 0, +kmax} (invalid d rows at the grid's ends, a negative carrier at -kmax) x PRN 1 and 32 (24 combinations,
    cycled), blocks 0 .. max_block.  Returns (tasks int32 [n][2], aid of `dtype`)"""
    combos = [(ca, lo, prn) for ca in (0, 1, spm // 2 - 1, spm - 1) for lo in (-kmax, 0, kmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    aid = np.zeros(n, dtype)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        aid[t] = (0, ca, lo, 0, ca / (spm * 1e3), lo * step_hz, 45.0)
        tasks[t] = (t % (max_block + 1), prn)
    return tasks, aid


def law_center(sat, m0, fs=FS, step_hz=STEP_HZ):
    """(ca_shift, lo_shift) the generator's law gives satellite `sat` at sample m0, floats (tests/aided_cases.py)"""
    cps = CPS * (1.0 + sat[2] / L1) / fs
    return ((m0 + sat[3]) * cps % 1023.0) / CPS * fs, sat[2] / step_hz


def weak_sats(amplitude=WEAK_AMPLITUDE):
    """the satellites in the gain scene's capture: STRONG and the weak one"""
    return STRONG + [(WEAK_SAT[0], amplitude) + WEAK_SAT[2:]]
