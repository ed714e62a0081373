"""Host side of the zero-acceleration harmonic-sum search (hd_accel_* in include/hipdedisp.h,
csrc/hd_accel.hip) and its numpy oracle (tests/accel_oracle.py): the interpolation taps, the
trials-corrected power threshold and the sigma of a hit against the closed form (and scipy
where it is installed), the oracle's physics (a half-bin tone, a comb in noise), the closest-r
merge against the oracle's on random lists, and the return codes that need no device.  CPU."""
import ctypes
import math

import numpy as np
import pytest

import accel_oracle as AO
from hipdedisp import Engine, PassParams, _lib
from hipdedisp import accel_stage as AS
from hipdedisp.synth import palfa_obs

STAGES = (1, 2, 4, 8, 16)
SIGMAS = (2.0, 3.0, 6.0)
NUMINDEP = 2.1e6                 # a PALFA spectrum's searched bins


def norm_sf(x):
    return 0.5 * math.erfc(x / math.sqrt(2.0))


def q_fsum(H, P):
    """Q(H, P) = e^-P sum_{k<H} P^k / k!, the terms summed exactly."""
    return math.exp(-P) * math.fsum(P ** k / math.factorial(k) for k in range(H))


def test_taps_bit_exact():
    want = np.array([np.float32(1.0 / (math.pi * (j - 0.5))) for j in range(1, 17)], np.float32)
    assert np.array_equal(AS.taps().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(AO.taps().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("H", STAGES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_powcut_closed_form(H, sigma):
    """numindep * Q(H, powcut) is the normal tail beyond sigma."""
    ni = NUMINDEP / H
    pc = AS.powcut(sigma, H, ni)
    assert ni * q_fsum(H, pc) == pytest.approx(norm_sf(sigma), rel=1e-12)
    assert pc == pytest.approx(AO.powcut(sigma, H, ni), rel=1e-14)


@pytest.mark.parametrize("H", STAGES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_powcut_matches_scipy(H, sigma):
    stats = pytest.importorskip("scipy.stats")
    ni = NUMINDEP / H
    want = stats.chi2.isf(stats.norm.sf(sigma) / ni, 2 * H) / 2.0
    assert AS.powcut(sigma, H, ni) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("H", STAGES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_sigma_round_trips_powcut(H, sigma):
    ni = NUMINDEP / H
    assert AS.sigma_of(AS.powcut(sigma, H, ni), H, ni) == pytest.approx(sigma, abs=1e-9)
    assert AO.sigma_of(AO.powcut(sigma, H, ni), H, ni) == pytest.approx(sigma, abs=1e-9)


@pytest.mark.parametrize("H", (1, 16))
def test_sigma_of_large_powers(H):
    """Powers of thousands (log p far below the smallest double): finite, increasing, and
    scipy's log-space inverse where it is installed."""
    ni = NUMINDEP / H
    s = [AS.sigma_of(p, H, ni) for p in (100.0, 500.0, 2000.0)]
    assert all(math.isfinite(x) for x in s) and s[0] < s[1] < s[2]
    assert s[0] > 8.0 and s[2] > 50.0
    for p, got in zip((100.0, 500.0, 2000.0), s):
        assert got == pytest.approx(AO.sigma_of(p, H, ni), abs=1e-9)
    assert AS.sigma_of(0.5, H, ni) == 0.0                     # p >= 0.5


@pytest.mark.parametrize("H", (1, 16))
def test_sigma_matches_scipy(H):
    special = pytest.importorskip("scipy.special")
    if not hasattr(special, "ndtri_exp"):
        pytest.skip("scipy.special.ndtri_exp needs scipy >= 1.9")
    ni = NUMINDEP / H
    for p in (30.0, 100.0, 500.0, 2000.0):
        # log Q from the closed form, the sum's leading power factored out
        logq = -p + (H - 1) * math.log(p) - math.lgamma(H) + math.log(
            math.fsum(math.exp(math.lgamma(H) - math.lgamma(k + 1) + (k - (H - 1)) * math.log(p)) for k in range(H)))
        logp = min(0.0, logq + math.log(ni))
        want = -special.ndtri_exp(logp) if logp < math.log(0.5) else 0.0      # (f): 0 when p >= 0.5
        assert AS.sigma_of(p, H, ni) == pytest.approx(want, abs=1e-9)


def test_oracle_half_bin_tone():
    """A noiseless tone at k + 0.5 keeps 1 - (4/pi^2) sum_{j>16} (j - 1/2)^-2 ~ 0.975 of its
    power in P[2k+1]; the integer bins beside it show 0.405."""
    numout, k, amp = 4096, 700, 30.0
    F = np.zeros((1, numout), np.float32)
    AO.add_tone(F[0], k + 0.5, amp, phase=0.3)
    P = AO.power_plane(F)[0]
    frac = float(P[2 * k + 1]) / amp ** 2
    assert 0.97 <= frac <= 1.0
    want = 1.0 - (4.0 / math.pi ** 2) * sum((j - 0.5) ** -2 for j in range(17, 200000))
    assert frac == pytest.approx(want, abs=2e-3)
    assert float(P[2 * k]) / amp ** 2 == pytest.approx(4.0 / math.pi ** 2, abs=1e-3)
    assert P[0] == 0.0 and P[1] == 0.0


def test_oracle_finds_comb_in_noise():
    numout, T = 16384, 10.0
    F = AO.noise_spectra(2, numout, seed=5)
    r0 = 411.5                                               # fundamental at a half bin
    AO.add_comb(F[1], r0, 8, 6.0)
    hits, cuts = AO.search(F, T, numharm=16, sigma=2.0, flo=2.0)
    assert set(cuts) == set(STAGES)
    h8 = hits[(hits["dm"] == 1) & (hits["numharm"] == 8)]
    assert len(h8)
    best = h8[np.argmax(h8["power"])]
    assert abs(int(best["r2"]) - int(round(2 * 8 * r0))) <= 1
    assert best["sigma"] > 10.0
    kept = AO.prune(hits)
    k1 = kept[kept["dm"] == 1]
    assert abs(float(k1["r2"][0]) / (2.0 * k1["numharm"][0]) - r0) <= 1.0


def random_hits(rng, n, ndm):
    h = np.empty(n, AO.HIT)
    h["dm"] = rng.integers(0, ndm, n)
    h["numharm"] = 1 << rng.integers(0, 5, n)
    h["r2"] = rng.integers(2, 4000, n)
    h["power"] = rng.random(n).astype(np.float32) * 50.0
    h["sigma"] = np.round(rng.random(n) * 12.0, 1)            # many equal sigmas
    return h


@pytest.mark.parametrize("seed,n,ndm", [(1, 0, 1), (2, 1, 1), (3, 300, 3), (4, 2000, 5)])
def test_prune_matches_oracle(seed, n, ndm):
    h = random_hits(np.random.default_rng(seed), n, ndm)
    if n >= 300:                                             # exact ties in every key but r2
        h[10:20] = h[10]
        h["r2"][10:20] = np.arange(500, 700, 20)
    got = AS.prune(h)
    want = AO.prune(h)
    assert got.tobytes() == want.tobytes()
    if n >= 300:
        assert 0 < len(got) < n
        f = AS.fundamentals(got)
        for d in range(ndm):
            fd = np.sort(f[got["dm"] == d])
            assert np.all(np.diff(fd) >= 15.0)


def test_search_return_codes_without_device():
    """hd_accel_search on a context without a device: HD_E_HIP; a numharm that is no stage:
    HD_E_INVAL; hd_set_fft needs the device too."""
    eng = Engine(_lib.HD_HOST_ONLY)
    try:
        eng.set_obs(palfa_obs(N=4096, nbits=8))
        p = eng.plan(PassParams(subdm=0.0, lodm=0.0, dmstep=0.1, numdms=4, nsub=96, ds=1, numout=4096))
        n = ctypes.c_int64()
        hits = np.empty(16, AS.HIT)
        hp = hits.ctypes.data_as(ctypes.c_void_p)
        L = eng._L
        assert L.hd_accel_search(p._p, 10.0, 2.0, 100.0, 16, 2.0, hp, 16, ctypes.byref(n), None) == _lib.HD_E_HIP
        for bad in (0, 3, 5, 32, -1):
            assert L.hd_accel_search(p._p, 10.0, 2.0, 100.0, bad, 2.0, hp, 16, ctypes.byref(n), None) == _lib.HD_E_INVAL
            assert "numharm" in _lib.last_error(eng._ctx)
        assert L.hd_accel_search(None, 10.0, 2.0, 100.0, 16, 2.0, hp, 16, ctypes.byref(n), None) == _lib.HD_E_INVAL
        spec = np.zeros((4, 4096), np.float32)
        assert L.hd_set_fft(p._p, 0, 4, spec.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == _lib.HD_E_HIP
        out = np.zeros(8, np.float32)
        assert L.hd_accel_get_powers(p._p, 0, 0, 8, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == _lib.HD_E_STATE
        p.destroy()
    finally:
        eng.close()


def test_host_argument_checks():
    L = _lib.load()
    v = ctypes.c_double()
    assert L.hd_accel_taps(None) == _lib.HD_E_INVAL
    assert L.hd_accel_powcut(2.0, 0, 100.0, ctypes.byref(v)) == _lib.HD_E_INVAL
    assert L.hd_accel_powcut(2.0, 4, 0.0, ctypes.byref(v)) == _lib.HD_E_INVAL
    assert L.hd_accel_sigma(10.0, 17, 100.0, ctypes.byref(v)) == _lib.HD_E_INVAL
    assert L.hd_accel_prune(None, 3, 15.0, ctypes.byref(ctypes.c_int64())) == _lib.HD_E_INVAL
