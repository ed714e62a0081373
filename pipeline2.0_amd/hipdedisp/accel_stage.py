"""The zero-acceleration periodicity search on a pass's device-resident spectra.

The reference runs, for every de-reddened .fft of a pass (lib/python/PALFA2_presto_search.py:
560-568, adding the wall time to job.lo_accelsearch_time):

    accelsearch -zmax 0 -numharm 16 -sigma 2.0 -flo 2.0 <fft>

(lo_accel_*: lib/python/config/searching_example.py:20-23).  Here the spectra hd_rednoise left
in HBM are searched where they are (hd_accel_search, csrc/hd_accel.hip): a half-bin power
plane by Fourier interpolation, incoherent sums of 1, 2, 4, 8 and 16 harmonics, a
trials-corrected power threshold per stage, and per 64 half bins the strongest sum above it;
only those hits come back, with their sigma, and the host merges the ones whose fundamentals
lie within 15 bins (hd_accel_prune).  [PRESTO-ext] restated (include/hipdedisp.h);
not covered: -zmax 50, candidate optimisation and -harmpolish, accelsearch's block-median
normalisation, the _ACCEL_0 / .cand / .txtcand files, sifting.  There is no CPU fallback.
"""
import ctypes
import time

import numpy as np

from . import _lib
from .engine import PrestoError

HIT = np.dtype([("dm", "<i4"), ("numharm", "<i4"), ("r2", "<i4"), ("power", "<f4"), ("sigma", "<f8")])
CLOSEST_R = 15.0            # accelsearch's ACCEL_CLOSEST_R [PRESTO-ext]
STAGES = (1, 2, 4, 8, 16)

_fp = ctypes.POINTER(ctypes.c_float)


def _host(rc, what):
    if rc:
        raise PrestoError("%s: %s" % (what, _lib.last_error()))


def taps():
    """The 16 float32 interpolation taps (hd_accel_taps)."""
    t = np.empty(16, np.float32)
    _host(_lib.load().hd_accel_taps(t.ctypes.data_as(_fp)), "hd_accel_taps")
    return t


def powcut(sigma, numharm, numindep):
    """Summed power of `numharm` harmonics whose chance over numindep trials is the normal
    tail beyond sigma (hd_accel_powcut)."""
    v = ctypes.c_double()
    _host(_lib.load().hd_accel_powcut(float(sigma), int(numharm), float(numindep), ctypes.byref(v)), "hd_accel_powcut")
    return v.value


def sigma_of(power, numharm, numindep):
    """Equivalent gaussian sigma of a summed power over numindep trials (hd_accel_sigma)."""
    v = ctypes.c_double()
    _host(_lib.load().hd_accel_sigma(float(power), int(numharm), float(numindep), ctypes.byref(v)), "hd_accel_sigma")
    return v.value


def set_fft(plan, packed, dm0=0):
    """hd_set_fft: packed spectra float32 [ndm][numout] into the plan's spectra buffer (the
    inverse of fft_stage.get_fft), e.g. from .fft files; the plan then owns the buffer."""
    a = np.ascontiguousarray(packed, np.float32)
    if a.ndim != 2 or a.shape[1] != plan.numout:
        raise ValueError("set_fft: spectra must be [ndm][numout = %d] float32" % plan.numout)
    plan.eng._chk(plan.eng._L.hd_set_fft(plan._p, int(dm0), int(a.shape[0]), a.ctypes.data_as(_fp)), "hd_set_fft")


def search(plan, T, numharm=16, sigma=2.0, flo=2.0, fhi=10000.0, cap=None, return_powcut=False):
    """hd_accel_search of the plan's spectra (T = numout * dt seconds): HIT records sorted by
    (dm, numharm, r2), sigma filled in; a candidate's fundamental is r2 / (2 numharm) bins.
    With return_powcut also the power thresholds of the five stages (0 where not searched)."""
    eng = plan.eng
    cap = int(cap if cap is not None else getattr(eng, "_acc_cap", 1 << 14))
    pc = (ctypes.c_double * 5)()
    while True:
        hits = np.empty(max(cap, 1), HIT)
        n = ctypes.c_int64()
        rc = eng._L.hd_accel_search(plan._p, float(T), float(flo), float(fhi), int(numharm), float(sigma),
                                    hits.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n), pc)
        if rc == _lib.HD_E_NOMEM and n.value > cap:              # room for every hit
            cap = int(n.value) + int(n.value) // 4
            eng._acc_cap = cap
            continue
        eng._chk(rc, "accelsearch -zmax 0")
        out = hits[:n.value]
        return (out, np.array(pc[:])) if return_powcut else out


def get_powers(plan, dm, q0=0, count=None):
    """P[q0 .. q0 + count) (half bins) of DM dm of the plan's last search (hd_accel_get_powers)."""
    if count is None:
        count = plan.numout - q0
    out = np.empty(int(count), np.float32)
    plan.eng._chk(plan.eng._L.hd_accel_get_powers(plan._p, int(dm), int(q0), int(count), out.ctypes.data_as(_fp)),
                  "hd_accel_get_powers")
    return out


def last_ms(plan):
    """(power plane ms, harmonic sums ms) on the device of the plan's last search."""
    a, b = ctypes.c_float(), ctypes.c_float()
    plan.eng._chk(plan.eng._L.hd_accel_last_ms(plan._p, ctypes.byref(a), ctypes.byref(b)), "hd_accel_last_ms")
    return a.value, b.value


def prune(hits, closest_r=CLOSEST_R):
    """hd_accel_prune: per DM in descending sigma, a hit is kept unless a kept one's
    fundamental lies within closest_r bins; the kept HIT records (DMs ascending, each DM's in
    descending sigma)."""
    a = np.array(hits, HIT)                                      # a copy: the library compacts in place
    n = ctypes.c_int64()
    _host(_lib.load().hd_accel_prune(a.ctypes.data_as(ctypes.c_void_p), len(a), float(closest_r), ctypes.byref(n)),
          "hd_accel_prune")
    return a[:n.value]


def fundamentals(hits):
    """Fundamental frequencies of HIT records, in bins (r2 / (2 numharm))."""
    return hits["r2"] / (2.0 * hits["numharm"])


def run_accel(plan, dt, numharm=16, sigma=2.0, flo=2.0, fhi=10000.0):
    """:560-568 for one pass: the pruned candidates of every DM; returns (seconds, HIT records)."""
    t0 = time.time()
    kept = prune(search(plan, plan.numout * dt, numharm, sigma, flo, fhi))
    return time.time() - t0, kept


def accel_pass(job, plan, ddplan, passnum, tempdir, opts):
    """search_stage hook: opts = dict(numharm=, sigma=, flo=, fhi=) (config.searching's
    lo_accel_*), optionally results=list, which receives (dm strings, kept HIT records) per
    pass.  Runs after fft_pass (the spectra must be in HBM); adds to job.lo_accelsearch_time."""
    t, kept = run_accel(plan, plan.sub_dt, opts.get("numharm", 16), opts.get("sigma", 2.0), opts.get("flo", 2.0),
                        opts.get("fhi", 10000.0))
    if opts.get("results") is not None:
        opts["results"].append((list(ddplan.dmlist[passnum]), kept))
    job.lo_accelsearch_time = getattr(job, "lo_accelsearch_time", 0.0) + t
    return t
