"""Reference of the observables tests: the model of include/gpsacq.h ("Observables") in Python integers and numpy.float64,
written from that text and not from the kernels, plus a forward simulator of fabricated tracking records (the channel model's NCO
bookkeeping only: the six sums are arbitrary numbers).

Nothing here loads the library except for the record dtypes."""
import numpy as np

M64 = (1 << 64) - 1
PERIOD = 1023 << 32                  # one code period of the prompt position, chips * 2^32
DIVISOR = 4393751543808000.0         # 1023 * 2^32 * 1000
WEEK_MS = 604800000
assert DIVISOR == float(PERIOD * 1000) and int(DIVISOR) == PERIOD * 1000


def time_tag(tow, bit_offset, bit_epoch0, eph_index):
    """(epoch, ms, eph, valid) of the model's TIME TAG"""
    assert 0 <= tow <= 100799
    return (bit_epoch0 + 20 * bit_offset, ((tow - 1) % 100800) * 6000, eph_index, 1)


def code_positions(samples, ca_rates, next_sample, ca_pos):
    """the backward recursion: [pos_0 .. pos_{n-1}] as Python integers mod 2^64"""
    n = len(samples)
    pos = [0] * n
    nxt, end = int(ca_pos), int(next_sample)
    for t in range(n - 1, -1, -1):
        n_t = (end - int(samples[t])) & M64
        nxt = (nxt + PERIOD - n_t * int(ca_rates[t])) & M64
        pos[t] = nxt
        end = int(samples[t])
    return pos


def position_at(samples, ca_rates, next_sample, pos, R):
    """(t, P) of receive sample R, or None when R lies outside the records"""
    n = len(samples)
    if n == 0 or R < int(samples[0]) or R >= int(next_sample):
        return None
    t = int(np.searchsorted(np.asarray(samples, np.uint64), np.uint64(R), side="right")) - 1
    end = int(samples[t + 1]) if t + 1 < n else int(next_sample)
    assert int(samples[t]) <= R < end
    return t, (pos[t] + (R - int(samples[t])) * int(ca_rates[t])) & M64


def observables(records, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix):
    """OBS_DTYPE [n_fix][n_chans] of the model.  records: TRACK_RECORD_DTYPE [n_chans][max_epochs], chans: TRACK_CHAN_DTYPE after
    the tracking call, tags: TIME_TAG_DTYPE."""
    import gpsacq
    n_chans = len(n_epochs)
    out = np.zeros((n_fix, n_chans), gpsacq.OBS_DTYPE)
    for c in range(n_chans):
        n = int(n_epochs[c])
        if not int(tags["valid"][c]) or n == 0:
            continue
        smp, rate = records["sample"][c, :n], records["ca_rate"][c, :n]
        nxt = int(chans["next_sample"][c])
        pos = code_positions(smp, rate, nxt, int(chans["ca_pos"][c]))
        first_epoch = int(chans["epoch"][c]) - n
        for i in range(n_fix):
            hit = position_at(smp, rate, nxt, pos, first_rx_sample + i * rx_step)
            if hit is None:
                continue
            t, P = hit
            assert P < PERIOD
            o = out[i, c]
            o["eph"], o["valid"], o["weight"] = int(tags["eph"][c]), 1, 1.0
            o["tx_ms"] = (int(tags["ms"][c]) + (first_epoch + t - int(tags["epoch"][c]))) % WEEK_MS
            o["tx_frac"] = np.float64(P) / np.float64(DIVISOR)  # P < 2^42: the conversion is exact, one IEEE division
    return out


def fabricate(seed, n, spm, first_sample=None, epoch0=None, prn=1, rate_span_hz=26.0):
    """Forward simulation of n epochs of a channel at spm samples per millisecond: n_t = ceil((1023 2^32 - ca_pos) / ca_rate),
    ca_pos += n_t ca_rate - 1023 2^32, ca_rate redrawn each epoch within +-rate_span_hz of nominal (0: constant).  Returns (records [n], the channel
    after them (shape (1,)), [ca_pos the channel had at the start of every epoch])."""
    import gpsacq
    rng = np.random.default_rng(seed)
    fs = spm * 1000.0
    nominal = int(1.023e6 / fs * 2 ** 32)
    span = int(rate_span_hz / fs * 2 ** 32)
    rec = np.zeros(n, gpsacq.TRACK_RECORD_DTYPE)
    ch = np.zeros(1, gpsacq.TRACK_CHAN_DTYPE)
    sample = int(rng.integers(0, 10 * spm)) if first_sample is None else int(first_sample)
    ca_pos = int(rng.integers(0, PERIOD))  # anywhere in the code: the first epoch is then a short one
    epoch = int(rng.integers(0, 5000)) if epoch0 is None else int(epoch0)
    walk = []
    for t in range(n):
        rate = nominal + int(rng.integers(-span, span + 1))
        n_t = -((ca_pos - PERIOD) // rate)  # ceil((PERIOD - ca_pos) / rate)
        walk.append(ca_pos)
        rec["sample"][t], rec["ca_rate"][t] = sample, rate
        rec["lo_rate"][t] = int(rng.integers(0, 1 << 32))
        for f in ("ie", "qe", "ip", "qp", "il", "ql"):
            rec[f][t] = int(rng.integers(-spm, spm + 1))
        ca_pos += n_t * rate - PERIOD
        assert 0 <= ca_pos < rate
        sample += n_t
    ch["prn"], ch["next_sample"], ch["ca_pos"], ch["epoch"] = prn, sample, ca_pos, epoch + n
    ch["ca_rate"] = nominal
    return rec, ch, walk
