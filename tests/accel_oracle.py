"""numpy restatement of the zero-acceleration harmonic-sum search (test helper; CPU).

The algorithm of include/hipdedisp.h's hd_accel_search block, steps (a)-(f), written so that
every float32 rounding the device makes is one numpy float32 operation here: the power plane
and the hit lists are compared bit for bit.  Thresholds and significances (c), (f) are double,
from the closed form Q(H, P) = e^-P sum_{k<H} P^k / k!.
"""
import math

import numpy as np

NTAPS = 16
STAGES = (1, 2, 4, 8, 16)
# sixteenths of r2 each stage adds, in order
STAGE_FRACS = {1: (), 2: (8,), 4: (4, 12), 8: (2, 6, 10, 14), 16: (1, 3, 5, 7, 9, 11, 13, 15)}
HIT = np.dtype([("dm", "<i4"), ("numharm", "<i4"), ("r2", "<i4"), ("power", "<f4"), ("sigma", "<f8")])


def taps():
    j = np.arange(1, NTAPS + 1, dtype=np.float64)
    return (1.0 / (np.pi * (j - 0.5))).astype(np.float32)


def power_plane(packed):
    """(a): packed spectra float32 [ndm][numout] -> P float32 [ndm][numout] (half bins)."""
    F = np.ascontiguousarray(packed, np.float32)
    ndm, numout = F.shape
    nb = numout // 2
    re = F[:, 0::2].copy()
    im = F[:, 1::2].copy()
    re[:, 0] = 0.0
    im[:, 0] = 0.0
    P = np.zeros((ndm, 2 * nb), np.float32)
    P[:, 0::2] = (re.astype(np.float64) * re.astype(np.float64) + im.astype(np.float64) * im.astype(np.float64)) \
        .astype(np.float32)
    t = taps()
    comp = []
    for x in (re, im):
        z = np.zeros((ndm, nb + 2 * NTAPS), np.float32)
        z[:, NTAPS:NTAPS + nb] = x                            # z[:, NTAPS + i] = F[i]
        acc = np.zeros((ndm, nb), np.float32)
        for j in range(1, NTAPS + 1):
            a = z[:, NTAPS + j:NTAPS + j + nb]
            b = z[:, NTAPS + 1 - j:NTAPS + 1 - j + nb]
            d = a - b                                         # float32
            m = t[j - 1] * d                                  # float32
            acc = acc + m                                     # float32
        comp.append(acc.astype(np.float64))
    P[:, 1::2] = (comp[0] * comp[0] + comp[1] * comp[1]).astype(np.float32)
    P[:, 0] = 0.0
    P[:, 1] = 0.0
    return P


def search_range(nb, T, flo, fhi):
    rlo = max(1, int(math.floor(flo * T)))
    rhi = min(int(math.floor(fhi * T)), nb - 1)
    return rlo, rhi


def harmonic_sums(Prow, rlo, rhi, numharm):
    """(b) for one DM: (r2 int64 [n], {H: S float32 [n]})."""
    r2 = np.arange(2 * rlo, 2 * rhi + 1, dtype=np.int64)
    S = Prow[r2].astype(np.float32)
    out = {1: S}
    for H in STAGES[1:]:
        if H > numharm:
            break
        for m in STAGE_FRACS[H]:
            S = S + Prow[(r2 * m + 8) >> 4]                   # float32 add chain
        out[H] = S
    return r2, out


def log_q(H, P):
    term, s = 1.0, 1.0
    for k in range(1, H):
        term = term * P / float(k)
        s += term
    return -P + math.log(s)


def log_sf(x):
    """log of the normal tail beyond x."""
    if x < 5.0:
        return math.log(0.5 * math.erfc(x / math.sqrt(2.0)))
    t = x
    for n in range(200 if x < 12.0 else 60, 0, -1):           # Mills ratio, continued fraction
        t = x + n / t
    return -0.5 * x * x - 0.5 * math.log(2.0 * math.pi) - math.log(t)


def _bisect_down(f, target, hi):
    """x with f(x) = target for a falling f, to the last bit (from above)."""
    lo = 0.0
    while f(hi) > target:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if f(mid) > target:
            lo = mid
        else:
            hi = mid
    return hi


def powcut(sigma, H, numindep):
    """(c)."""
    target = log_sf(sigma) - math.log(numindep)
    if not target < 0.0:
        return 0.0
    return _bisect_down(lambda p: log_q(H, p), target, 64.0)


def sigma_of(power, H, numindep):
    """(f)."""
    if not power > 0.0 or not math.isfinite(power):
        return 0.0
    logp = min(0.0, log_q(H, power) + math.log(numindep))
    if not logp < math.log(0.5):
        return 0.0
    return _bisect_down(log_sf, logp, 8.0)


def search(packed, T, numharm=16, sigma=2.0, flo=2.0, fhi=10000.0, P=None):
    """(a)-(d), (f): HIT records sorted by (dm, numharm, r2), and the stages' powcut."""
    if P is None:
        P = power_plane(packed)
    ndm, nb = P.shape[0], P.shape[1] // 2
    rlo, rhi = search_range(nb, T, flo, fhi)
    assert rlo < rhi
    stages = [H for H in STAGES if H <= numharm]
    cuts = {H: powcut(sigma, H, (rhi - rlo) / float(H)) for H in stages}
    rows = []
    for d in range(ndm):
        r2, sums = harmonic_sums(P[d], rlo, rhi, numharm)
        blk = r2 >> 6
        for H in stages:
            S = sums[H]
            above = np.nonzero(S > np.float32(cuts[H]))[0]
            if not len(above):
                continue
            # per aligned block of 64 half bins: the largest S, the lowest r2 among equals
            starts = np.nonzero(np.diff(blk[above], prepend=-1))[0]
            for a, b in zip(starts, list(starts[1:]) + [len(above)]):
                idx = above[a:b]
                i = idx[np.argmax(S[idx])]                    # first maximum
                rows.append((d, H, int(r2[i]), S[i], sigma_of(float(S[i]), H, (rhi - rlo) / float(H))))
    hits = np.array(rows, HIT) if rows else np.empty(0, HIT)
    hits = hits[np.lexsort((hits["r2"], hits["numharm"], hits["dm"]))]
    return hits, cuts


def prune(hits, closest_r=15.0):
    """(e): per DM in descending sigma (ties: lower numharm, lower r2), keep unless a kept
    one's fundamental lies within closest_r bins."""
    order = sorted(range(len(hits)), key=lambda i: (int(hits["dm"][i]), -float(hits["sigma"][i]),
                                                    int(hits["numharm"][i]), int(hits["r2"][i])))
    kept = []
    for i in order:
        d = int(hits["dm"][i])
        f = float(hits["r2"][i]) / (2.0 * float(hits["numharm"][i]))
        ok = True
        for k in kept:
            if int(hits["dm"][k]) == d and abs(float(hits["r2"][k]) / (2.0 * float(hits["numharm"][k])) - f) < closest_r:
                ok = False
                break
        if ok:
            kept.append(i)
    return hits[kept] if kept else hits[:0]


def noise_spectra(ndm, numout, seed):
    """Packed spectra of unit-mean exponential noise power (complex gaussian bins); bin 0 =
    (1, 0) as hd_rednoise leaves it."""
    rng = np.random.default_rng(seed)
    F = (rng.standard_normal((ndm, numout)) * math.sqrt(0.5)).astype(np.float32)
    F[:, 0], F[:, 1] = 1.0, 0.0
    return F


def add_tone(Frow, r, amp, phase=0.0):
    """A sinusoid of Fourier amplitude amp at frequency r bins (any real r) added to one packed
    spectrum: the response amp sinc(pi (k - r)) e^{i (phase - pi (k - r))} on the 64 bins around r."""
    nb = len(Frow) // 2
    k0 = int(math.floor(r))
    for k in range(max(1, k0 - 31), min(nb, k0 + 33)):
        x = math.pi * (k - r)
        s = 1.0 if abs(x) < 1e-12 else math.sin(x) / x
        Frow[2 * k] += np.float32(amp * s * math.cos(phase - x))
        Frow[2 * k + 1] += np.float32(amp * s * math.sin(phase - x))


def add_comb(Frow, r0, nharm, amp, phase=0.0):
    """Harmonics 1 .. nharm of a fundamental at r0 bins, equal amplitudes."""
    for h in range(1, nharm + 1):
        add_tone(Frow, r0 * h, amp, phase + 0.7 * h)
