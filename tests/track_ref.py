"""An independent reference of one tracking channel, written in numpy / Python from the text "THE CHANNEL MODEL" in
include/gpsacq.h.  It shares no bit tricks with tests/c/track_model.c or csrc/track_kernels.hip:

* the carrier signs are the signs of cos and -sin of 2 pi ph / 2^32 in float64 (with an explicit tie rule at the four
  exact quarter points, where float64 cannot decide a sign);
* the early / prompt / late chips are read at real chip positions P, P + 1/2, P - 1/2 reduced mod 1023, from the oracle's C/A
  generator (track_helpers.chip_words), not from the engine's table;
* the loops run in Python integers, reduced mod 2^64 explicitly, with shifts written as multiplications by 2**k and ">> 32"
  as a floor division of the reduced value.

The samples are either 1-bit (v_i = 1 - 2 x, v_q = 0) or the complex integers of "Tracking channels on an 8-bit IQ capture"
(v = byte - off - dc on both arms): one sum routine, I_X = sum h_X (v_i C - v_q S), Q_X = sum h_X (v_i S + v_q C), serves both.

audit() checks what a call of gpsacq_track or gpsacq_track_iq8 (or their CPU models) wrote for one channel: every epoch's geometry, its six sums,
the loop arithmetic that took each record to the next, the final state field by field and why the call stopped.  It returns
the branches the channel went through, so that tests can assert they reached what they aim at."""
import numpy as np

from track_helpers import chip_words

TWO32, TWO63, TWO64 = 2 ** 32, 2 ** 63, 2 ** 64
FULL = 1023 * TWO32                     # one code period, chips * 2^32
AID_RATIO = 1540                        # L1 / 1.023 MHz
_QUARTER = TWO32 // 4
_chips = {}


def chips(prn):
    """the 1023 chips of `prn` as 0/1 (1 = chip value -1)"""
    if prn not in _chips:
        w = chip_words(prn)
        _chips[prn] = np.unpackbits(w.view(np.uint8), bitorder="little")[:1023].astype(np.int8)
    return _chips[prn]


def carrier_signs(ph):
    """(cos bit, sin bit) of uint32 phases `ph` (int64 array): 1 where cos(2 pi ph / 2^32), resp. -sin(2 pi ph / 2^32), is
    negative.  ph / 2^32 is exact in float64 and away from the quarter points |cos|, |sin| >= sin(2 pi / 2^32) ~ 1.5e-9, far above
    the rounding of np.cos / np.sin, so the float64 sign is the true one.  Tie rule at the quarter points, where the value is an
    exact zero (float64 gives +-6e-17 instead): the sign is the one the function takes just after the point, at increasing phase
    -- the half-open quadrants [0, 1/4), [1/4, 1/2), ... of the header's bit formulas.  So cos at 1/4 counts negative and at 3/4
    positive; -sin at 0 counts negative and at 1/2 positive."""
    x = ph.astype(np.float64) * (2.0 * np.pi / TWO32)
    cos_neg = np.cos(x) < 0.0
    sin_neg = -np.sin(x) < 0.0
    cos_neg = np.where(ph == _QUARTER, True, np.where(ph == 3 * _QUARTER, False, cos_neg))
    sin_neg = np.where(ph == 0, True, np.where(ph == 2 * _QUARTER, False, sin_neg))
    return cos_neg.astype(np.int8), sin_neg.astype(np.int8)


def code_chips(P, prn):
    """chips (0/1) at early, prompt and late of prompt positions P (int64, chips * 2^32, in [0, 1023 * 2^32)): the positions
    P + 1/2 and P - 1/2 chip as real numbers (exact in float64: P < 2^42), reduced mod 1023, floored."""
    c = chips(prn)
    p = P.astype(np.float64) / TWO32
    idx = [np.floor(np.mod(p + d, 1023.0)).astype(np.int64) for d in (0.5, 0.0, -0.5)]
    return [c[i] for i in idx]


def _sums(samples, base, prn, starts, ns, lo_phase, lo_rate, ca_pos, ca_rate, chunk_samples):
    """I_X = sum h_X (v_i C - v_q S), Q_X = sum h_X (v_i S + v_q C), X in E, P, L, of epochs given by their start sample, length and
    NCO state (int arrays); samples(at) gives (v_i, v_q) of the samples base + at as integer arrays (v_q None: 0, the 1-bit
    channel).  |v| <= 256 and an epoch has at most 65535 samples, so every sum is below 2^26 and exact as a float64 bincount.
    Returns int64 [n_epochs][6]."""
    starts, ns = np.asarray(starts, np.int64), np.asarray(ns, np.int64)
    out = np.zeros((starts.size, 6), np.int64)
    a = 0
    while a < starts.size:
        b = a + 1
        tot = int(ns[a])
        while b < starts.size and tot + int(ns[b]) <= chunk_samples:
            tot += int(ns[b])
            b += 1
        n = ns[a:b]
        ep = np.repeat(np.arange(b - a), n)
        j = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
        at = np.repeat(starts[a:b] - base, n) + j
        ph = (np.asarray(lo_phase[a:b], np.int64)[ep] + j * np.asarray(lo_rate[a:b], np.int64)[ep]) % TWO32
        P = np.asarray(ca_pos[a:b], np.int64)[ep] + j * np.asarray(ca_rate[a:b], np.int64)[ep]
        assert (P < FULL).all()
        cb, sb = carrier_signs(ph)
        C, S = 1 - 2 * cb, 1 - 2 * sb  # int8; the products below stay within +-512: int8 for 1-bit samples, int16 for 8-bit ones
        xi, xq = samples(at)
        if xq is None:
            re_, im_ = xi * C, xi * S
        else:
            re_, im_ = xi * C - xq * S, xi * S + xq * C
        for k, ch in enumerate(code_chips(P, prn)):
            h = 1 - 2 * ch
            out[a:b, 2 * k] = np.bincount(ep, weights=h * re_, minlength=b - a).astype(np.int64)
            out[a:b, 2 * k + 1] = np.bincount(ep, weights=h * im_, minlength=b - a).astype(np.int64)
        a = b
    return out


def epoch_sums(samples01, first_sample, prn, starts, ns, lo_phase, lo_rate, ca_pos, ca_rate, chunk_samples=1 << 21):
    """The six sums (IE, QE, IP, QP, IL, QL) of epochs given by their start sample, length and NCO state (int arrays);
    samples01: the window's samples, 0/1 (1 = negative): v_i = 1 - 2 x, v_q = 0.  Returns int64 [n_epochs][6]."""
    return _sums(lambda at: (1 - 2 * samples01[at].astype(np.int8), None), first_sample, prn, starts, ns, lo_phase, lo_rate, ca_pos, ca_rate, chunk_samples)


def iq_samples(iq, signed, dc_i, dc_q):
    """(v_i, v_q) of interleaved I, Q bytes, "Tracking channels on an 8-bit IQ capture": v = byte - off - dc, off = 128 for unsigned
    bytes and 0 for two's-complement ones.  int16 arrays (|v| <= 256)."""
    raw = np.asarray(iq).view(np.uint8).astype(np.int16).reshape(-1, 2)
    a = np.where(raw >= 128, raw - 256, raw) if signed else raw - 128
    return a[:, 0] - np.int16(dc_i), a[:, 1] - np.int16(dc_q)


def epoch_sums_iq(iq, first_sample, signed, dc_i, dc_q, prn, starts, ns, lo_phase, lo_rate, ca_pos, ca_rate, chunk_samples=1 << 21):
    """epoch_sums for a window of complex integer samples: iq holds samples first_sample .. as interleaved I, Q bytes."""
    pairs = np.asarray(iq).view(np.uint8).ravel()
    pairs = pairs[:pairs.size // 2 * 2].reshape(-1, 2)
    return _sums(lambda at: iq_samples(pairs[at], signed, dc_i, dc_q), first_sample, prn, starts, ns, lo_phase, lo_rate, ca_pos, ca_rate, chunk_samples)


def _signed(v):
    v %= TWO64
    return v - TWO64 if v >= TWO63 else v


def _u64(v):
    return int(v) % TWO64


def _p(params, name):
    return int(params[name] if isinstance(params, dict) else getattr(params, name))


def audit(bits, first_sample, chan0, params, records, n_epochs, chan_out, max_epochs=None, prompt=None, sum_epochs=None, seed=0, iq=None):
    """Check one channel's call of gpsacq_track over the window bits (uint8, samples first_sample ..), or, with iq = (signed, dc_i,
    dc_q), of gpsacq_track_iq8 in multi-bit mode over the window of interleaved I, Q bytes passed as `bits` (it ends at
    first_sample + len(bits) // 2, any sample): chan0 / chan_out are its
    TRACK_CHAN_DTYPE record before and after, records its TRACK_RECORD_DTYPE rows (at least n_epochs), prompt its [epochs][2]
    rows if that output was written.  sum_epochs: recompute the sums of every epoch (None) or of that many seeded ones.
    Raises AssertionError on the first disagreement; returns the branches taken:
      agc_down / agc_up (gain_adj 0 -> -1 / -1 -> 0), agc_polls, ring_wraps, fll_epochs, costas_epochs, costas_adj_epochs (with
      gain_adj = -1), aid (epochs where the aid fired), lost (set of window terms 'lo_int', 'lo_rate', 'ca_int', 'ca_rate', or
      'min_epoch' / 'max_epoch'), stop ('window', 'max_epochs', 'lost', 'entered_lost'), short_first (first epoch shorter than a
      period: it started away from chip 0), late_wrap / early_wrap (epochs whose late / early position wrapped)."""
    c0 = chan0
    prn = int(c0["prn"])
    end = first_sample + (8 * len(bits) if iq is None else len(bits) // 2)
    rep = dict(agc_down=0, agc_up=0, agc_polls=0, ring_wraps=0, fll_epochs=0, costas_epochs=0, costas_adj_epochs=0, aid=[], lost=set(),
               stop=None, short_first=False, late_wrap=0, early_wrap=0, epochs=int(n_epochs))
    lo_ki, lo_kp, ca_ki, ca_kp, fll_k = (_p(params, k) for k in ("lo_ki", "lo_kp", "ca_ki", "ca_kp", "fll_k"))
    agc_period, aid_epoch = _p(params, "agc_period"), _p(params, "aid_epoch")
    agc_lo, agc_hi, lo_win, ca_win = (_p(params, k) for k in ("agc_lo", "agc_hi", "lo_window", "ca_window"))
    min_ep, max_ep = _p(params, "min_epoch"), _p(params, "max_epoch")

    status = int(c0["status"])
    ns_ = int(c0["next_sample"])
    lo_phase, lo_rate, ca_pos, ca_rate = int(c0["lo_phase"]), int(c0["lo_rate"]), int(c0["ca_pos"]), int(c0["ca_rate"])
    lo_int, ca_int = _u64(c0["lo_int"]), _u64(c0["ca_int"])
    lo_nom, ca_nom = _u64(c0["lo_nom"]), _u64(c0["ca_nom"])
    epoch, gain_adj, pwr_pos = int(c0["epoch"]), int(c0["gain_adj"]), int(c0["pwr_pos"])
    pwr = [int(v) for v in c0["pwr"]]
    prev_ip, prev_qp, fll_left = int(c0["prev_ip"]), int(c0["prev_qp"]), int(c0["fll_left"])

    n_epochs = int(n_epochs)
    if status != 0:
        assert n_epochs == 0, "a LOST channel ran %d epochs" % n_epochs
        assert chan_out.tobytes() == c0.tobytes(), "a LOST channel changed"
        rep["stop"] = "entered_lost"
        return rep
    rec = records[:n_epochs]
    r_sample, r_lo, r_ca = rec["sample"].tolist(), rec["lo_rate"].tolist(), rec["ca_rate"].tolist()
    sums = np.stack([rec[k] for k in ("ie", "qe", "ip", "qp", "il", "ql")], axis=1).astype(np.int64) if n_epochs else np.zeros((0, 6), np.int64)
    sl = sums.tolist()
    geo = np.zeros((n_epochs, 6), np.int64)  # start, n, lo_phase, lo_rate, ca_pos, ca_rate
    lost = set()
    for t in range(n_epochs):
        assert not lost
        n = -(-(FULL - ca_pos) // ca_rate)
        assert min_ep <= n <= max_ep, (t, n)
        assert r_sample[t] == ns_ and r_lo[t] == lo_rate and r_ca[t] == ca_rate, ("record", t, r_sample[t], ns_, r_lo[t], lo_rate, r_ca[t], ca_rate)
        assert ns_ + n <= end, (t, "epoch beyond the window")
        if t == 0 and ca_pos >= ca_rate:
            rep["short_first"] = True
        if ca_pos < TWO32 // 2:
            rep["late_wrap"] += 1
        if ca_pos + (n - 1) * ca_rate >= FULL - TWO32 // 2:
            rep["early_wrap"] += 1
        geo[t] = (ns_, n, lo_phase, lo_rate, ca_pos, ca_rate)
        IE, QE, IP, QP, IL, QL = sl[t]
        lo_phase = (lo_phase + n * lo_rate) % TWO32
        ca_pos = ca_pos + n * ca_rate - FULL
        assert 0 <= ca_pos < ca_rate
        ns_ += n
        epoch += 1
        k = epoch
        if agc_period > 0 and k % agc_period == 0:
            rep["agc_polls"] += 1
            pwr[pwr_pos] = IP * IP + QP * QP
            pwr_pos = (pwr_pos + 1) % 8
            rep["ring_wraps"] += pwr_pos == 0
            S = sum(pwr)
            if gain_adj != 0:
                if S < 8 * agc_lo:
                    gain_adj = 0
                    rep["agc_up"] += 1
            elif S > 8 * agc_hi:
                gain_adj = -1
                rep["agc_down"] += 1
        if fll_left > 0:
            dot = prev_ip * IP + prev_qp * QP
            cross = prev_ip * QP - prev_qp * IP
            e = (1 if dot > 0 else -1 if dot < 0 else 0) * cross
            lo_int = (lo_int + e * 2 ** fll_k) % TWO64
            lo_rate = lo_int // TWO32
            fll_left -= 1
            rep["fll_epochs"] += 1
        else:
            e = IP * QP
            lo_int = (lo_int + e * 2 ** (lo_ki + gain_adj)) % TWO64
            lo_rate = ((lo_int + e * 2 ** (lo_kp + gain_adj)) % TWO64) // TWO32
            rep["costas_epochs"] += 1
            rep["costas_adj_epochs"] += gain_adj != 0
        prev_ip, prev_qp = IP, QP
        e = (IE * IE + QE * QE) - (IL * IL + QL * QL)
        ca_int = (ca_int + e * 2 ** ca_ki) % TWO64
        ca_rate = ((ca_int + e * 2 ** ca_kp) % TWO64) // TWO32
        if k == aid_epoch:
            lo_int = (lo_nom + (_signed(ca_int - ca_nom)) * AID_RATIO) % TWO64
            lo_rate = lo_int // TWO32
            rep["aid"].append(k)
        for name, v, nom, w in (("lo_int", lo_int, lo_nom, lo_win), ("lo_rate", lo_rate * TWO32, lo_nom, lo_win),
                                ("ca_int", ca_int, ca_nom, ca_win), ("ca_rate", ca_rate * TWO32, ca_nom, ca_win)):
            if abs(_signed(v - nom)) > w:
                lost.add(name)
    if lost:
        status = 1
        rep["stop"] = "lost"
    elif max_epochs is not None and n_epochs == max_epochs:
        rep["stop"] = "max_epochs"
    else:
        assert ca_rate > 0
        n = -(-(FULL - ca_pos) // ca_rate)
        if n < min_ep or n > max_ep:
            status = 1
            lost.add("min_epoch" if n < min_ep else "max_epoch")
            rep["stop"] = "lost"
        else:
            assert ns_ + n > end, "the call stopped although the next epoch fits the window"
            rep["stop"] = "window"
    rep["lost"] = lost
    want = dict(prn=prn, status=status, next_sample=ns_, lo_phase=lo_phase, lo_rate=lo_rate, lo_int=_signed(lo_int), ca_pos=ca_pos,
                ca_rate=ca_rate, epoch=epoch, ca_int=_signed(ca_int), lo_nom=_signed(lo_nom), ca_nom=_signed(ca_nom), gain_adj=gain_adj,
                pwr_pos=pwr_pos, prev_ip=prev_ip, prev_qp=prev_qp, fll_left=fll_left, reserved=int(c0["reserved"]))
    for f, v in want.items():
        assert int(chan_out[f]) == v, ("final state", f, int(chan_out[f]), v)
    assert [int(v) for v in chan_out["pwr"]] == pwr, ("final state", "pwr")
    if prompt is not None and n_epochs:
        assert np.array_equal(np.asarray(prompt[:n_epochs], np.int64), sums[:, 2:4]), "prompt differs from the records"
    # the six sums
    if n_epochs:
        sel = np.arange(n_epochs)
        if sum_epochs is not None and sum_epochs < n_epochs:
            sel = np.sort(np.random.default_rng(seed).choice(n_epochs, sum_epochs, replace=False))
        lo = int(geo[sel, 0].min()) - first_sample
        hi = int((geo[sel, 0] + geo[sel, 1]).max()) - first_sample
        g = geo[sel]
        if iq is None:
            b0, b1 = lo // 8, (hi + 7) // 8
            s01 = np.unpackbits(np.asarray(bits[b0:b1], np.uint8), bitorder="little")
            got = epoch_sums(s01, first_sample + 8 * b0, prn, g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5])
        else:
            got = epoch_sums_iq(np.asarray(bits).view(np.uint8).ravel()[2 * lo:2 * hi], first_sample + lo, iq[0], iq[1], iq[2], prn,
                                g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5])
        bad = np.nonzero((got != sums[sel]).any(axis=1))[0]
        assert bad.size == 0, ("sums", int(sel[bad[0]]), got[bad[0]].tolist(), sums[sel[bad[0]]].tolist())
    return rep
