"""The case table of the generator tests (tests/test_gen_ref.py on the CPU, tests/test_gpu_generate.py on the GPU) and the glue
between a generated buffer and tests/gen_ref.py: what is compared, what is left out, what counts as a disagreement.

A case is a dict: kind ("bits": Engine.generate, "iq": Engine.generate_iq8), group, name, the engine's (fc, fs), sats
[(prn, amplitude, doppler_hz, code_phase_samples, carrier_phase_cycles)], sigma, seed, first (sample), n (bytes for "bits", samples
for "iq"), nav (None or [n_sats][n_nav_bits] of +-1) and, for "iq", if_hz, scale, signed.  No case has more than 2^20 samples.

Rate A is fc = 4.092 MHz, fs = 5.456 MHz: fc / fs = 3/4 and, at Doppler 0, 3/16 chip per sample, both exact in binary.  Rate B is
fc = 0.62 MHz, fs = 2.8 MHz, where neither is."""
import numpy as np

import gen_ref

RATE_A, RATE_B = (4.092e6, 5.456e6), (0.62e6, 2.8e6)
FOUR = [(3, 0.2, 1234.5, 100.25, 0.3), (17, 0.151, -3100.0, 4000.0, 0.9), (5, 0.12, 2501.0, -12.25, 0.0), (9, 0.3, -9000.0, 7000.5, -1.3)]
TWO = FOUR[:2]
TWELVE = [(prn, 0.1 + 0.02 * k, -5500.0 + 1000.0 * k, 431.3 * k - 900.0, 0.083 * k - 0.4)
          for k, prn in enumerate((1, 2, 4, 7, 8, 11, 13, 19, 23, 29, 31, 32))]
K16 = 1 << 16


def _bits(group, name, sats, sigma, n_bytes, rate=RATE_A, seed=1, first=0, nav=None, exact=False):
    return dict(kind="bits", group=group, name=name, fc=rate[0], fs=rate[1], sats=list(sats), sigma=sigma, seed=seed, first=first,
                n=n_bytes, nav=nav, exact=exact)


def _iq(group, name, sats, sigma, n, rate=RATE_A, seed=1, first=0, nav=None, if_hz=0.0, scale=16.0, signed=True, exact=False):
    return dict(kind="iq", group=group, name=name, fc=rate[0], fs=rate[1], sats=list(sats), sigma=sigma, seed=seed, first=first, n=n,
                nav=nav, if_hz=if_hz, scale=scale, signed=signed, exact=exact)


def _nav_rows(n_sats, n_nav, seed):
    """+-1 rows in which neighbouring bits, the last and the first included, differ where a boundary is looked at"""
    nav = np.where(np.random.default_rng(seed).integers(0, 2, (n_sats, n_nav)) > 0, 1, -1).astype(np.int8)
    if n_nav == 1:
        nav[:, 0] = (-1, 1)[:n_sats]
    else:
        nav[:, 0], nav[:, -1] = 1, -1
        if n_nav == 3:
            nav[:, 1] = (1, -1)[:n_sats]       # satellite 0: + + - (bits 199 and 200 are its second and third), satellite 1: + - -
    return nav


def _table():
    t = []
    # ---- 1-bit ------------------------------------------------------------------------------------------------------------------
    for n in (1, 255, 256, 257, 8192):       # the tail byte and the edge of a 256-thread workgroup
        t.append(_bits("lengths", "noise-%d" % n, [], 1.0, n, seed=11))
        t.append(_bits("lengths", "two-%d" % n, TWO, 1.0, n, seed=12))
    for first, n in ((0, 8192), (8, 8192), (2 ** 32 - 8, 4096), (2 ** 40, 8192)):   # the third window crosses 2^32
        t.append(_bits("starts", "first-%d" % first, TWO, 1.0, n, seed=13, first=first))
    # Noise-free single-satellite sweep: the full product of PRN x Doppler x code phase x carrier phase x rate, less one corner:
    # Doppler 0 with code phase 0.  There the code position is m * 3/16 (rate A) or m * 1023/2800 (rate B) but for the rounding of
    # the rate, so every 16th, or every 2800th, sample sits on a chip edge and the rule of gen_ref leaves out more than the 1e-4
    # that tests/test_gen_ref.py allows.  Doppler 0 keeps the other three code phases and code phase 0 the other two Dopplers; the
    # exact chip grid of rate A is what "ties" predicts by hand.
    # At rate B the carriers of Doppler 0 and -10 000 Hz are 31/140 and 61/280 cycle per sample and every theta of the sweep is a
    # multiple of 1/10, so on 2 samples of every 140, or 280, the cosine is zero but for rounding: those fall inside tau.
    for r, rate in (("A", RATE_A), ("B", RATE_B)):
        for prn in (1, 32):
            for dop in (-10000.0, 0.0, 7654.3):
                for cp in (0.0, -0.5, -16368.75, 1000000.75):
                    for th in (0.3, -1.3, 7.9):
                        if dop == 0.0 and cp == 0.0:
                            continue
                        t.append(_bits("sweep", "%s-prn%d-d%g-c%g-t%g" % (r, prn, dop, cp, th), [(prn, 1.0, dop, cp, th)], 0.0, K16 // 8, rate))
    # Exact ties: fc / fs = 3/4, Doppler 0.  On every odd sample the cosine is exactly 0; the code position (m - 1/2) * 3/16 is
    # never an integer.
    for th in (0.0, 0.5):
        t.append(_bits("ties", "theta-%g" % th, [(7, 1.0, 0.0, -0.5, th)], 0.0, K16 // 8, exact=True))
    # Navigation bits, two satellites with rows of their own.  "negative": q < 0 over the first 5000 samples.  "boundary": the
    # window lies across q = 200 * 20460 of satellite 0 (sample 21 824 000 at 3/16 chip per sample, less Doppler and code phase).
    for n_nav in (1, 3, 50):
        sats = [(6, 1.0, 1500.0, -5000.5, 0.2), (21, 0.7, -2200.0, -77.25, 0.6)]
        t.append(_bits("nav", "negative-%d" % n_nav, sats, 0.0, K16 // 8, nav=_nav_rows(2, n_nav, 100 + n_nav)))
        t.append(_bits("nav", "boundary-%d" % n_nav, sats, 0.0, K16 // 8, first=21824000 - K16 // 2, nav=_nav_rows(2, n_nav, 200 + n_nav)))
    t.append(_bits("twelve", "twelve", TWELVE, 0.0, K16 // 8))
    t.append(_bits("noisy", "sigma1-seed0-2^20", FOUR, 1.0, (1 << 20) // 8, seed=0))
    t.append(_bits("noisy", "sigma1-seed77", FOUR, 1.0, K16 // 8, seed=77))
    t.append(_bits("noisy", "sigma1-seed2^63+5", FOUR, 1.0, K16 // 8, seed=2 ** 63 + 5))
    t.append(_bits("noisy", "sigma0.25-seed77", FOUR, 0.25, K16 // 8, seed=77))
    t.append(_bits("noisy", "sigma0.25-seed0-B", FOUR, 0.25, K16 // 8, RATE_B, seed=0))
    # ---- 8-bit ------------------------------------------------------------------------------------------------------------------
    for n in (1, 255, 256, 257):
        t.append(_iq("iq-lengths", "n-%d" % n, TWO, 1.0, n, seed=21, if_hz=250e3))
    t.append(_iq("iq-lengths", "first-12345", TWO, 1.0, 4097, seed=22, first=12345, if_hz=250e3))
    t.append(_iq("iq-lengths", "first-2^32-3", TWO, 1.0, 4097, seed=23, first=2 ** 32 - 3, if_hz=250e3, signed=False))
    # Ties of rint: carrier 1 + 0j on every sample, so I = chip * amplitude and Q = 0.  0.5 -> 0, 1.5 -> 2, 2.5 -> 2.
    for amp in (0.5, 1.5, 2.5):
        for signed in (True, False):
            t.append(_iq("iq-rint", "amp-%g-%s" % (amp, "s8" if signed else "u8"), [(12, amp, 0.0, -0.5, 0.0)], 0.0, 4096, scale=1.0,
                         signed=signed, exact=True))
    for signed in (True, False):
        t.append(_iq("iq-clamp", "clamp-%s" % ("s8" if signed else "u8"), [(25, 10.0, 3001.7, 10.25, 0.1)], 0.0, K16, if_hz=250e3,
                     scale=16.0, signed=signed))
    for if_hz in (250e3, -250e3):            # Q carries +sin: the spectrum sense
        t.append(_iq("iq-sense", "if%+g" % if_hz, [(30, 1.0, 1234.5, 333.4, 0.15)], 0.0, K16, RATE_B, if_hz=if_hz, scale=100.0))
    t.append(_iq("iq-noisy", "plain", FOUR, 1.0, 1 << 18, seed=31, if_hz=250e3))
    t.append(_iq("iq-noisy", "nav", FOUR, 1.0, 1 << 18, seed=32, if_hz=-250e3, signed=False, nav=_nav_rows(4, 50, 300)))
    for c in t:
        if c["nav"] is not None:
            c["nav"].setflags(write=False)
    names = [c["group"] + "/" + c["name"] for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _table()
GROUPS = ("lengths", "starts", "sweep", "ties", "nav", "twelve", "noisy", "iq-lengths", "iq-rint", "iq-clamp", "iq-sense", "iq-noisy")


def cases(group=None, kind=None):
    return [c for c in CASES if (group is None or c["group"] == group) and (kind is None or c["kind"] == kind)]


def case_id(c):
    return c["group"] + "/" + c["name"]


def n_samples(c):
    return 8 * c["n"] if c["kind"] == "bits" else c["n"]


_refs = {}


def reference(c, law=None):
    """gen_ref's answer for case c.  The right law's is computed once, shared and never written to."""
    if law is None:
        key = case_id(c)
        if key not in _refs:
            _refs[key] = reference(c, gen_ref.LAW)
            for v in _refs[key].values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return _refs[key]
    if c["kind"] == "bits":
        return law.bits(c["fc"], c["fs"], c["sats"], c["sigma"], c["seed"], c["first"], 8 * c["n"], c["nav"])
    return law.iq8(c["fs"], c["sats"], c["if_hz"], c["scale"], c["sigma"], c["seed"], c["first"], c["n"], c["nav"])


def decided(c, ref):
    """[n] or [n][2] bool: the reference decides this value -- outside the left-out mask and outside the margin"""
    if c["kind"] == "bits":
        return ~ref["skip"] & (np.abs(ref["y"]) > ref["tau"])
    half = np.abs(ref["v"] - np.floor(ref["v"]) - 0.5)            # distance from the nearest half-integer
    return ~ref["skip"][:, None] & (half > ref["margin"][:, None])


def expected(c, ref, law=gen_ref.LAW):
    """what the generator should write: bits 0/1 per sample, or [n][2] bytes"""
    if c["kind"] == "bits":
        return (ref["y"] < 0.0).astype(np.uint8)
    return law.quantise(ref["v"], c["signed"])


def samples(c, out):
    """the generator's output as bits 0/1 per sample, or [n][2] bytes"""
    if c["kind"] == "bits":
        return gen_ref.unpack(out)
    return np.asarray(out).reshape(-1, 2)


def compare(c, got, ref=None, want=None):
    """got: samples(c, output).  Returns dict(compared, left_out, in_margin, differ_in_margin, bad, worst, off_by_more): `bad` counts decided values
    that differ from the reference's, `worst` is the smallest |y_ref| (1-bit) or the largest distance from a half-integer (8-bit)
    among them, `off_by_more` counts undecided 8-bit values further than 1 from the reference's (undecided bits may be anything)."""
    ref = reference(c) if ref is None else ref
    want = expected(c, ref) if want is None else want
    dec = decided(c, ref)
    wrong = got != want
    bad = dec & wrong
    r = dict(compared=int(dec.sum()), left_out=int(ref["skip"].sum()) * (1 if c["kind"] == "bits" else 2),
             in_margin=int((~dec).sum()) - int(ref["skip"].sum()) * (1 if c["kind"] == "bits" else 2), bad=int(bad.sum()), worst=None,
             off_by_more=0, differ_in_margin=int((wrong & ~dec & ~(ref["skip"] if c["kind"] == "bits" else ref["skip"][:, None])).sum()))
    if c["kind"] == "bits":
        if r["bad"]:
            r["worst"] = float(np.abs(ref["y"])[bad].min())
    else:
        if r["bad"]:
            r["worst"] = float(np.abs(ref["v"] - np.floor(ref["v"]) - 0.5)[bad].max())
        r["off_by_more"] = int((~dec & ~ref["skip"][:, None] & (np.abs(got.astype(np.int16) - want.astype(np.int16)) > 1)).sum())
    return r


def hand(c):
    """The output of an exact case predicted by hand, in Python integers: samples(c, output) must equal it everywhere.  Both
    groups use one satellite at rate A, Doppler 0 and code phase -1/2: the chip count is floor((m - 1/2) * 3/16) =
    (6 m - 3) // 32 and (6 m - 3) / 32 is never an integer.
    ties: the carrier phase is 3 m / 4 + theta: cos = 0 on odd m (bit 0), +1, -1, +1 ... on m = 0, 2, 4 ... (theta = 1/2: the
    opposite), and the bit is (chip * cos < 0).
    iq-rint: the carrier is 1 + 0 j, so I = rint(amplitude * chip) with 1/2 -> 0, 3/2 -> 2, 5/2 -> 2 and Q = 0."""
    import track_ref
    (prn, amp, dop, cp, th), = c["sats"]
    assert c["exact"] and (c["fc"], c["fs"]) == RATE_A and dop == 0.0 and cp == -0.5 and c["first"] == 0 and c["sigma"] == 0.0 and c["nav"] is None
    ca = track_ref.chips(prn)
    chip = [1 - 2 * int(ca[((6 * m - 3) // 32) % 1023]) for m in range(n_samples(c))]
    if c["group"] == "ties":
        flip = {0.0: 1, 0.5: -1}[th]
        return np.array([0 if m % 2 else int(chip[m] * flip * (1, -1)[(m // 2) % 2] < 0) for m in range(len(chip))], np.uint8)
    assert c["group"] == "iq-rint" and c["if_hz"] == 0.0 and th == 0.0 and c["scale"] == 1.0
    mag = {0.5: 0, 1.5: 2, 2.5: 2}[amp]
    iq = np.zeros((len(chip), 2), np.int16)
    iq[:, 0] = np.array(chip) * mag
    return iq.astype(np.int8) if c["signed"] else (iq + 128).astype(np.uint8)


def report(c, r):
    return "%-34s %8d compared, %6d left out, %6d inside the margin (%d of them differ), %d disagreements%s%s" % (
        case_id(c), r["compared"], r["left_out"], r["in_margin"], r["differ_in_margin"], r["bad"],
        "" if r["worst"] is None else (", the %s %.3g" % ("smallest |y_ref| among them" if c["kind"] == "bits" else "furthest of them from a half-integer by", r["worst"])),
        "" if not r["off_by_more"] else ", %d undecided values off by more than 1" % r["off_by_more"])
