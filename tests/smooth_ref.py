"""Reference of the smoothing tests: the model of include/gpsacq.h ("Carrier-smoothed observables") in Python integers and
numpy.float64, written from that text and not from the kernels.

  * the per-instant quantities: usable, t, P, A(R), Z, the phase-lock test;
  * segments and the window sum D_i two ways -- the direct sum of int64 differences and the prefix difference mod 2^64;
  * the two records of every instant;
  * a lane-by-lane restatement of the chunk / run / scan / carry indexing the header prescribes for k_smooth_scan;
  * fabricated records whose code and carrier move together.

Nothing here loads the library except for the record dtypes."""
import numpy as np

import obs_ref
import rate_ref

M64 = (1 << 64) - 1
FULL = 1023 << 32
AID = 1540
RESET, UNLOCKED, FULLW = 1, 2, 4
INVALID, RAW, LOCKED = 0, 1, 2
DEFAULTS = dict(window=1000, lock_epochs=20, lock_num=1, lock_den=2, jump=385 << 32, invert=0, reserved=0)
s64 = rate_ref.s64


def par(params=None, **over):
    """a dict of Python integers from None (the defaults), a dict or a SMOOTH_PARAMS_DTYPE record"""
    out = dict(DEFAULTS)
    if params is not None:
        if isinstance(params, dict):
            out.update({k: int(v) for k, v in params.items()})
        else:
            rec = np.asarray(params).ravel()[0]
            out.update({k: int(rec[k]) for k in rec.dtype.names})
    out.update({k: int(v) for k, v in over.items()})
    return out


def params_valid(p):
    return (1 <= p["window"] <= 65536 and 0 <= p["lock_epochs"] <= 1024 and 1 <= p["lock_num"] <= p["lock_den"] <= 1024 and p["jump"] >= 0)


def lock_sums(ip, qp):
    """([LN_0 .. LN_n], [LD_0 .. LD_n]): the sums over u < t of ip^2 - qp^2 and ip^2 + qp^2, mod 2^64"""
    ln, ld = [0], [0]
    for a, b in zip(ip, qp):
        a, b = int(a), int(b)
        ln.append((ln[-1] + a * a - b * b) & M64)
        ld.append((ld[-1] + a * a + b * b) & M64)
    return ln, ld


def locked(ln, ld, t, p):
    L = p["lock_epochs"]
    if L == 0:
        return True
    if t < L - 1:
        return False
    N, D = s64(ln[t + 1] - ln[t + 1 - L]), s64(ld[t + 1] - ld[t + 1 - L])
    return D > 0 and s64(N * p["lock_den"]) >= s64(D * p["lock_num"])


def channel_series(rec, n, chan, tag, nom_word, first_rx_sample, rx_step, n_fix, p, per_epoch=None):
    """per instant of ONE channel: (state [n_fix], t, P, Z) as lists of Python integers; Z = 0 where the instant is not locked.
    rec: TRACK_RECORD_DTYPE [max_epochs], chan a TRACK_CHAN_DTYPE record, tag a TIME_TAG_DTYPE record.  per_epoch: a dict that
    keeps the channel's per-epoch sums (pos_t, A_t, the lock sums) between calls on the same records."""
    state, tt, PP, ZZ = [INVALID] * n_fix, [0] * n_fix, [0] * n_fix, [0] * n_fix
    n = int(n)
    if n == 0 or not int(tag["valid"]):
        return state, tt, PP, ZZ
    smp, nxt = rec["sample"][:n], int(chan["next_sample"])
    if per_epoch is None or "sums" not in per_epoch:
        sums = (obs_ref.code_positions(smp, rec["ca_rate"][:n], nxt, int(chan["ca_pos"])),
                rate_ref.carrier_acc(smp, rec["lo_rate"][:n], nxt, int(nom_word)), lock_sums(rec["ip"][:n], rec["qp"][:n]))
        if per_epoch is not None:
            per_epoch["sums"] = sums
    pos, acc, (ln, ld) = sums if per_epoch is None else per_epoch["sums"]
    cw = ((int(chan["ca_nom"]) & M64) >> 32) & 0xFFFFFFFF
    first_epoch = int(chan["epoch"]) - n
    S = int(smp[0])
    sgn = -1 if p["invert"] else 1
    R_all = [first_rx_sample + i * rx_step for i in range(n_fix)]
    t_all = np.searchsorted(np.asarray(smp, np.uint64), np.array([min(R, M64) for R in R_all], np.uint64), side="right") - 1
    for i, R in enumerate(R_all):
        if R < S or R >= nxt:
            continue
        t = int(t_all[i])
        dt = R - int(smp[t])
        P = (pos[t] + dt * int(rec["ca_rate"][t])) & M64
        A = acc[t] + dt * rate_ref.d_word(rec["lo_rate"][t], nom_word)
        tt[i], PP[i] = t, P
        if locked(ln, ld, t, p):
            state[i] = LOCKED
            ZZ[i] = (AID * ((first_epoch + t) * FULL + P - (R - S) * cw) - sgn * A) & M64
        else:
            state[i] = RAW
    return state, tt, PP, ZZ


def segment_starts(state, Z, jump):
    """s_i at every locked instant (None elsewhere)"""
    seg, cur = [None] * len(state), None
    for i, st in enumerate(state):
        if st != LOCKED:
            continue
        if i == 0 or state[i - 1] != LOCKED or (jump > 0 and abs(s64(Z[i] - Z[i - 1])) > jump):
            cur = i
        seg[i] = cur
    return seg


def prefix(Z):
    """[S_0 .. S_n] mod 2^64"""
    S = [0]
    for v in Z:
        S.append((S[-1] + v) & M64)
    return S


def window_sum_direct(Z, i, m):
    """D_i as the sum of the int64 differences, an unbounded Python integer"""
    return sum(s64(Z[j] - Z[i]) for j in range(i - m + 1, i + 1))


def window_sum_prefix(S, Z, i, m):
    """D_i as the prefix difference mod 2^64, read as int64"""
    return s64((S[i + 1] - S[i + 1 - m]) - m * Z[i])


def smooth_channel(state, tt, PP, ZZ, chan_epoch_first, tag, p, direct=False):
    """the two records of every instant of one channel: a list of (obs fields, info fields) dicts"""
    n_fix = len(state)
    seg = segment_starts(state, ZZ, p["jump"])
    S = prefix(ZZ)
    out = []
    for i in range(n_fix):
        if state[i] == INVALID:
            out.append(None)
            continue
        P, k = PP[i], 0
        info = dict(window=0, flags=UNLOCKED, cmc=0, corr=0)
        if state[i] == LOCKED:
            s = seg[i]
            m = min(i - s + 1, p["window"])
            D = s64(window_sum_direct(ZZ, i, m)) if direct else window_sum_prefix(S, ZZ, i, m)
            q = D // m
            c = q // AID
            Pp = P + c
            k = Pp // FULL
            P = Pp - k * FULL
            info = dict(window=m, flags=(RESET if s == i else 0) | (FULLW if m == p["window"] else 0), cmc=s64(ZZ[i] - ZZ[s]), corr=q)
        assert 0 <= P < FULL
        obs = dict(eph=int(tag["eph"]), valid=1, weight=1.0,
                   tx_ms=(int(tag["ms"]) + (chan_epoch_first + tt[i] + k - int(tag["epoch"]))) % obs_ref.WEEK_MS,
                   tx_frac=np.float64(P) / np.float64(obs_ref.DIVISOR))
        out.append((obs, info))
    return out


def smooth_observables(records, n_epochs, chans, tags, nom_words, first_rx_sample, rx_step, n_fix, params=None, direct=False, cache=None):
    """(OBS_DTYPE [n_fix][n_chans], SMOOTH_INFO_DTYPE [n_fix][n_chans]) of the model.  cache: a dict the caller keeps for ONE set of
    records, channels, tags and nominal words; calls that differ in the window or the jump alone then share the per-instant series."""
    import gpsacq
    p = par(params)
    assert params_valid(p)
    n_chans = len(n_epochs)
    obs = np.zeros((n_fix, n_chans), gpsacq.OBS_DTYPE)
    info = np.zeros((n_fix, n_chans), gpsacq.SMOOTH_INFO_DTYPE)
    for c in range(n_chans):
        n = int(n_epochs[c])
        key = (c, first_rx_sample, rx_step, n_fix, p["lock_epochs"], p["lock_num"], p["lock_den"], p["invert"])
        if cache is not None and key in cache:
            series = cache[key]
        else:
            series = channel_series(records[c], n, chans[c], tags[c], int(nom_words[c]), first_rx_sample, rx_step, n_fix, p,
                                    per_epoch=None if cache is None else cache.setdefault(("epochs", c), {}))
            if cache is not None:
                cache[key] = series
        hits = smooth_channel(*series, int(chans["epoch"][c]) - n, tags[c], p, direct=direct)
        for k in obs.dtype.names:
            obs[k][:, c] = [0 if h is None else h[0].get(k, 0) for h in hits]
        for k in info.dtype.names:
            info[k][:, c] = [0 if h is None else h[1][k] for h in hits]
    return obs, info


def scan_lanes(Z, state, jump, lanes=64, run=4):
    """k_smooth_scan's numbers by its prescribed indexing: chunks of lanes * run instants, each lane taking `run` consecutive
    instants plus the one before its run, an inclusive sum scan and an inclusive max scan over the lanes by doubling offsets, a
    64-bit carry and a carried latest start between chunks.  Returns ([S_0 .. S_n], [s_i]) with s_i = -1 before the first start."""
    n = len(Z)
    S, seg = [None] * (n + 1), [None] * n
    S[0] = 0
    carry, carry_seg = 0, -1
    chunk = lanes * run
    for base in range(0, n, chunk):
        pre = [[0] * run for _ in range(lanes)]
        sg = [[-1] * run for _ in range(lanes)]
        tot, tot_seg = [0] * lanes, [-1] * lanes
        for lane in range(lanes):
            i0 = base + lane * run
            get = lambda i: (Z[i], state[i]) if 0 <= i < n else (0, INVALID)
            acc, cur = 0, -1
            for j in range(run):
                (zp, sp), (z, st) = get(i0 + j - 1), get(i0 + j)
                acc = (acc + z) & M64
                d = s64(z - zp)
                if st == LOCKED and (sp != LOCKED or (jump > 0 and (d > jump or d < -jump))):
                    cur = i0 + j
                pre[lane][j], sg[lane][j] = acc, cur
            tot[lane], tot_seg[lane] = acc, cur
        incl, incl_seg = list(tot), list(tot_seg)
        off = 1
        while off < lanes:
            incl = [(incl[l] + incl[l - off]) & M64 if l >= off else incl[l] for l in range(lanes)]
            incl_seg = [max(incl_seg[l], incl_seg[l - off]) if l >= off else incl_seg[l] for l in range(lanes)]
            off <<= 1
        for lane in range(lanes):
            left = (carry + incl[lane] - tot[lane]) & M64
            left_seg = max(carry_seg, incl_seg[lane - 1]) if lane > 0 else carry_seg
            for j in range(run):
                i = base + lane * run + j
                if i < n:
                    S[i + 1] = (left + pre[lane][j]) & M64
                    seg[i] = max(sg[lane][j], left_seg)
        carry = (carry + incl[lanes - 1]) & M64
        carry_seg = max(carry_seg, incl_seg[lanes - 1])
    return S, seg


def fabricate_coherent(seed, n, spm, fc=4.092e6, k_span=40, noise=0, jump_at=None, jump_words=0, **kw):
    """obs_ref.fabricate's records with code and carrier moving together: per epoch an integer k, ca_rate = cw + k (+ a noise word
    of up to +-noise, and jump_words more in epoch jump_at: a code slip), lo_rate = nom + 1540 k, so that with noise = 0
    code-minus-carrier is constant.  The channel's ca_nom / lo_nom hold cw and nom.  Returns (records [n], channel (1,), nom_word)."""
    rng = np.random.default_rng(seed)
    fs = spm * 1000.0
    cw = int(1.023e6 / fs * 2 ** 32)
    nom = int(fc / fs * 2 ** 32) & 0xFFFFFFFF
    rec, ch, _ = obs_ref.fabricate(seed, n, spm, rate_span_hz=0.0, **kw)
    ks = rng.integers(-k_span, k_span + 1, n)
    wob = rng.integers(-noise, noise + 1, n) if noise else np.zeros(n, np.int64)
    if jump_at is not None and 0 <= jump_at < n:
        wob[jump_at] += jump_words
    sample = int(rec["sample"][0]) if n else 0
    # replay the channel model forward with the new rates from the position the fabricated channel started at
    pos_start = obs_ref.code_positions(rec["sample"], rec["ca_rate"], int(ch["next_sample"][0]), int(ch["ca_pos"][0]))[0] if n else 0
    ca_pos = pos_start
    for t in range(n):
        rate = cw + int(ks[t]) + int(wob[t])
        n_t = -((ca_pos - FULL) // rate)
        rec["sample"][t], rec["ca_rate"][t] = sample, rate
        rec["lo_rate"][t] = (nom + AID * int(ks[t])) & 0xFFFFFFFF
        ca_pos += n_t * rate - FULL
        sample += n_t
    ch["next_sample"], ch["ca_pos"] = sample, ca_pos if n else int(ch["ca_pos"][0])
    ch["ca_nom"], ch["lo_nom"] = cw << 32, s64(nom << 32)
    # a prompt a Costas loop in lock would show: all of the power in IP
    rec["ip"] = np.where(rng.integers(0, 2, n) > 0, 1, -1) * (spm // 4)
    rec["qp"] = rng.integers(-spm // 64, spm // 64 + 1, n)
    return rec, ch, nom


def fabricate_case(seed, spm, n_chans, n=600):
    """The records of the fabricated GPU cases: n_chans coherent channels of n epochs with per-epoch noise on ca_rate, and, where
    n_chans allows, a planted code slip of 0.6 chip (channel 0, epoch n // 2: spread over that epoch, so of two instants a
    millisecond apart one sees at least 0.3 chip of it), an unlocked stretch (qp large, channels 0 and 2,
    epochs n // 4 .. n // 4 + 60), a channel with 0 epochs (channel 1) and an invalid tag (the last of four or more channels).
    Returns (records [n_chans][n + 5], n_epochs, chans, tags, nom_words)."""
    import gpsacq
    rec = np.zeros((n_chans, n + 5), gpsacq.TRACK_RECORD_DTYPE)
    chans = np.zeros(n_chans, gpsacq.TRACK_CHAN_DTYPE)
    tags = np.zeros(n_chans, gpsacq.TIME_TAG_DTYPE)
    ne = np.zeros(n_chans, np.int32)
    nom = np.zeros(n_chans, np.uint32)
    slip = int(0.6 * 2 ** 32 / spm)  # code words per sample that move the code 0.6 chip in one epoch
    for c in range(n_chans):
        nc = 0 if (c == 1 and n_chans > 1) else n - 7 * c
        r, ch, w = fabricate_coherent(seed + 17 * c, nc, spm, noise=3000, jump_at=n // 2 if c == 0 else None, jump_words=slip,
                                      first_sample=40 * spm + 13 * c, epoch0=1000 + 50 * c, prn=c + 1)
        if c in (0, 2) and nc:
            a = n // 4
            r["qp"][a:a + 60], r["ip"][a:a + 60] = spm // 3, spm // 50
        rec[c, :nc], chans[c], ne[c], nom[c] = r, ch[0], nc, w
        tags[c] = (900 + 20 * c, 604799000 + 100 * c if c % 2 else 5000 * c, c, 0 if (c == n_chans - 1 and n_chans >= 4) else 1)
    return rec, ne, chans, tags, nom
