"""GPU zero-acceleration harmonic-sum search (hd_accel_search, csrc/hd_accel.hip) against
tests/accel_oracle.py: the half-bin power plane and the hit lists bit for bit, on crafted
spectra uploaded with hd_set_fft (unit-mean exponential noise plus harmonic combs at integer
and half bins, at the top and the bottom edge of the search range) at two series geometries
(numout 16384 with 3 DMs; 17496 = 2^3 3^7 with 5 DMs, so numout/2 is no multiple of 64), the
capacity and ownership contracts, and end to end on the injected-pulsar beam of
test_gpu_candidates.py reduced to 2^16 spectra.  Parity with PRESTO unpinned."""
import ctypes
import json
import os

import numpy as np
import pytest

import accel_oracle as AO
import fft_oracle as FO
import oracle as OR
from hipdedisp import Opts, PassParams, PrestoError, _lib
from hipdedisp import accel_stage as AS
from hipdedisp import fft_stage as FS
from hipdedisp import plan
from hipdedisp.synth import host_spectra, palfa_obs, palfa_synth, rfifind_ptsperint, synth_mask

HERE = os.path.dirname(os.path.abspath(__file__))
T_CRAFT = 10.0                    # seconds the crafted spectra stand for: flo 2.0 -> rlo 20, 2 rlo = 40
GEOMS = {16384: 3, 17496: 5}      # numout -> DMs


def crafted_spectra(numout, ndm):
    """Seeded noise plus per-DM combs (fundamental in bins, harmonics, amplitude)."""
    nb = numout // 2
    F = AO.noise_spectra(ndm, numout, seed=numout)
    rlo, rhi = AO.search_range(nb, T_CRAFT, 2.0, 10000.0)
    assert rhi == nb - 1
    combs = [(0, 300.0, 16, 5.0),                             # integer bins
             (1, 411.5, 8, 5.0),                              # half bins
             (2, (nb - 1) / 16.0, 16, 5.0),                   # the 16th harmonic is the last searchable bin
             (0, (rlo + 1) / 16.0, 16, 5.0)]                  # the fundamental just above rlo / 16
    if ndm > 3:
        combs += [(3, 123.25, 4, 6.0), (4, 1000.5, 2, 7.0), (4, 77.0, 1, 8.0)]
    for d, r0, nh, amp in combs:
        AO.add_comb(F[d], r0, nh, amp)
    return F


@pytest.fixture(scope="module")
def oracle_planes():
    """The crafted spectra of both geometries and the oracle's power planes, computed once."""
    out = {}
    for numout, ndm in GEOMS.items():
        F = crafted_spectra(numout, ndm)
        out[numout] = (F, AO.power_plane(F))
    return out


@pytest.fixture(scope="module")
def craft_engine(engine):
    engine.set_obs(palfa_obs(N=16384, nbits=8), Opts())
    return engine


def make_plan(eng, numout, subdm=10.0):
    pp = PassParams(subdm=subdm, lodm=subdm - 5.0, dmstep=0.5, numdms=GEOMS[numout], nsub=96, ds=1, numout=numout)
    p = eng.plan(pp)
    FS.prepare(p)
    return p


def assert_hits_equal(dev, ora):
    assert len(dev) == len(ora), (len(dev), len(ora))
    for f in ("dm", "numharm", "r2"):
        assert np.array_equal(dev[f], ora[f]), f
    assert np.array_equal(dev["power"].view(np.uint32), ora["power"].view(np.uint32))
    np.testing.assert_allclose(dev["sigma"], ora["sigma"], rtol=0, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("numout", sorted(GEOMS))
def test_power_plane_bit_exact(craft_engine, oracle_planes, numout):
    F, P = oracle_planes[numout]
    p = make_plan(craft_engine, numout)
    try:
        AS.set_fft(p, F)
        assert np.array_equal(FS.get_fft(p), F)               # hd_set_fft is hd_get_fft's inverse
        AS.search(p, T_CRAFT, numharm=1)
        for d in range(GEOMS[numout]):
            got = AS.get_powers(p, d)
            assert got.shape == (numout,)
            bad = np.nonzero(got.view(np.uint32) != P[d].view(np.uint32))[0]
            assert len(bad) == 0, (d, bad[:5], got[bad[:5]], P[d][bad[:5]])
        assert np.array_equal(AS.get_powers(p, 1, 2 * 411, 8), P[1][822:830])
        with pytest.raises(PrestoError):
            AS.get_powers(p, 0, numout - 4, 8)
    finally:
        p.destroy()


CASES = [
    # numharm, sigma, flo, fhi
    (1, 2.0, 2.0, 10000.0),
    (4, 2.0, 2.0, 10000.0),
    (16, 2.0, 2.0, 10000.0),       # 2 rlo = 40: the first block starts inside a wave
    (16, 2.0, 3.2, 10000.0),       # 2 rlo = 64: on a block boundary
    (16, 2.0, 2.0, 500.03),        # fhi below Nyquist: rhi = 5000
    (16, -1.0, 2.0, 10000.0),      # the lowest useful threshold
]


@pytest.mark.gpu
@pytest.mark.parametrize("numout", sorted(GEOMS))
def test_hits_bit_exact(craft_engine, oracle_planes, numout):
    F, P = oracle_planes[numout]
    p = make_plan(craft_engine, numout)
    try:
        AS.set_fft(p, F)
        for numharm, sigma, flo, fhi in CASES:
            dev, pc = AS.search(p, T_CRAFT, numharm, sigma, flo, fhi, return_powcut=True)
            ora, cuts = AO.search(F, T_CRAFT, numharm, sigma, flo, fhi, P=P)
            print("numout %d numharm %d sigma %g flo %g fhi %g: %d device hits, %d oracle hits"
                  % (numout, numharm, sigma, flo, fhi, len(dev), len(ora)))
            for i, H in enumerate(AO.STAGES):
                assert pc[i] == cuts.get(H, 0.0)
            assert_hits_equal(dev, ora)
            assert len(dev) > 0                               # the combs are found
        # every comb at its place in the numharm 16 list
        dev = AS.search(p, T_CRAFT, 16, 2.0, 2.0, 10000.0)
        top = dev[(dev["dm"] == 2) & (dev["numharm"] == 16)]
        assert 2 * (numout // 2 - 1) in top["r2"]             # the last searchable half bin
        low = dev[(dev["dm"] == 0) & (dev["numharm"] == 16)]
        assert low["r2"].min() <= 2 * 21 + 1                  # the comb at the bottom edge
    finally:
        p.destroy()


@pytest.mark.gpu
def test_dense_hits_append_and_sort(craft_engine, oracle_planes):
    """Thousands of hits (the noise scaled to 9 times the power the threshold assumes): the
    atomic append past the device list's first size, and the sort."""
    numout = 17496
    F = (oracle_planes[numout][0] * np.float32(3.0)).astype(np.float32)
    F[:, 0], F[:, 1] = 1.0, 0.0
    p = make_plan(craft_engine, numout)
    try:
        AS.set_fft(p, F)
        dev = AS.search(p, T_CRAFT, 16, 2.0, 2.0, 10000.0, cap=64)
        ora, _ = AO.search(F, T_CRAFT, 16, 2.0, 2.0, 10000.0)
        print("dense: %d hits" % len(dev))
        assert len(dev) > 3000
        assert_hits_equal(dev, ora)
    finally:
        p.destroy()


@pytest.mark.gpu
def test_cap_contract(craft_engine, oracle_planes):
    numout = 16384
    F, P = oracle_planes[numout]
    ora, _ = AO.search(F, T_CRAFT, 16, 2.0, 2.0, 10000.0, P=P)
    assert len(ora) > 4
    p = make_plan(craft_engine, numout)
    try:
        AS.set_fft(p, F)
        hits = np.zeros(4, AS.HIT)
        n = ctypes.c_int64()
        rc = craft_engine._L.hd_accel_search(p._p, T_CRAFT, 2.0, 10000.0, 16, 2.0, hits.ctypes.data_as(ctypes.c_void_p),
                                             4, ctypes.byref(n), None)
        assert rc == _lib.HD_E_NOMEM
        assert n.value == len(ora)
        assert not hits["numharm"].any()                      # nothing copied
        assert_hits_equal(AS.search(p, T_CRAFT, 16, 2.0, 2.0, 10000.0, cap=len(ora)), ora)
    finally:
        p.destroy()


@pytest.mark.gpu
def test_state_errors(craft_engine, oracle_planes):
    numout = 16384
    F, _ = oracle_planes[numout]
    p1, p2 = make_plan(craft_engine, numout, 10.0), make_plan(craft_engine, numout, 30.0)
    try:
        with pytest.raises(PrestoError, match="HD_E_STATE"):
            AS.search(p1, T_CRAFT)                            # no spectra yet
        AS.set_fft(p1, F)
        AS.search(p1, T_CRAFT)
        AS.set_fft(p2, F)                                     # the second plan takes the buffer over
        with pytest.raises(PrestoError, match="HD_E_STATE"):
            AS.search(p1, T_CRAFT)
        with pytest.raises(PrestoError, match="HD_E_INVAL"):
            AS.search(p2, T_CRAFT, flo=900.0)                 # rlo >= rhi
        with pytest.raises(PrestoError, match="HD_E_INVAL"):
            AS.search(p2, T_CRAFT, numharm=3)
        assert len(AS.search(p2, T_CRAFT))
        with pytest.raises(PrestoError, match="HD_E_STATE"):
            AS.get_powers(p1, 0)                              # the plane now holds p2's search
        assert AS.get_powers(p2, 0, 0, 2).tolist() == [0.0, 0.0]
    finally:
        p1.destroy()
        p2.destroy()


# ---- end to end: the injected-pulsar beam of test_gpu_candidates.py at 2^16 spectra ----------
N_BEAM = 1 << 16


def zaplist():
    g = json.load(open(os.path.join(HERE, "golden", "palfa_zaplist.json")))
    return [tuple(b) for b in g["birdies"]]


def reduced_beam():
    obs = palfa_obs(N=N_BEAM, nbits=8)
    s = palfa_synth()
    pts = rfifind_ptsperint(obs.dt)
    mask, pad = synth_mask(obs, s, pts)
    d0 = plan.ddplans_for("pdev")[0]
    k = next(i for i in range(d0.numpasses) if float(d0.dmlist[i][0]) <= 71.0 <= float(d0.dmlist[i][-1]))
    pp = PassParams(subdm=float(d0.subdmlist[k]), lodm=float(d0.lodm_arg(k)), dmstep=float(d0.dmstep_arg()),
                    numdms=d0.dmsperpass, nsub=d0.numsub, ds=1, numout=plan.choose_N(N_BEAM))
    return obs, s, pts, mask, pad, pp


def pulsar_kept(kept, pp, T):
    """Kept candidates whose fundamental is within 1 bin of the 4.6 ms pulsar's, at a DM within
    1.5 of 71."""
    f0 = T / 0.0046
    f = kept["r2"] / (2.0 * kept["numharm"])
    dm = pp.lodm + kept["dm"] * pp.dmstep
    return kept[(np.abs(f - f0) <= 1.0) & (np.abs(dm - 71.0) <= 1.5)]


def test_reduced_beam_shows_pulsar_on_oracle_path():
    """CPU: the end-to-end case's premise -- at 2^16 spectra the oracle's own series, FFT, zap
    and rednoise still leave the pulsar's fundamental among the pruned candidates."""
    obs, s, pts, mask, pad, pp = reduced_beam()
    raw = host_spectra(obs, s)
    _, x = OR.run_pass(obs, Opts(), raw, pp, mask=mask, ptsperint=pts, padvals=pad, omp=True)
    T = pp.numout * obs.dt
    nb = pp.numout // 2
    F = FO.realfft(x).astype(np.complex64)
    F = FO.zap(F, FO.zap_ranges(*FO.birdie_bins(zaplist(), T), nb))
    F = FO.rednoise(F, FO.rednoise_blocks(nb, T))
    packed = np.ascontiguousarray(F).view(np.float32)
    hits, _ = AO.search(packed, T)
    found = pulsar_kept(AO.prune(hits), pp, T)
    assert len(found)
    assert found["sigma"].max() > 5.0


@pytest.mark.gpu
def test_end_to_end_pulsar_candidate(engine):
    obs, s, pts, mask, pad, pp = reduced_beam()
    engine.set_obs(obs, Opts())
    engine.synth_device(s)
    engine.set_mask(mask, pts, pad)
    p = engine.plan(pp)
    try:
        p.run_subband()
        p.run_dedisp(to_host=False)
        T = p.numout * p.sub_dt
        FS.realfft(p)
        FS.zapbirds(p, *FS.birdie_bins(zaplist(), T))
        FS.rednoise(p, T)
        dev = AS.search(p, T)
        packed = FS.get_fft(p)
    finally:
        p.destroy()
        engine.set_mask()
    ora, _ = AO.search(packed, T)
    assert_hits_equal(dev, ora)
    kept = AS.prune(dev)
    assert kept.tobytes() == AO.prune(dev).tobytes()
    found = pulsar_kept(kept, pp, T)
    assert len(found)
    assert found["sigma"].max() > 5.0


@pytest.mark.gpu
def test_search_stage_accel_option(engine, tmp_path):
    """search_stage.run_pass(accel=...) after fft=: the pass's pruned candidates equal the
    oracle's from the .fft files the FFT stage wrote, and the seconds go to
    job.lo_accelsearch_time (PALFA2_presto_search.py:567)."""
    import copy
    from hipdedisp.formats import psrfits
    from hipdedisp.search_stage import DedispJob, dedisperse_job, run_pass
    obs = palfa_obs(N=8192, nbits=8, nsblk=512)
    fn = str(tmp_path / "beam.fits")
    psrfits.write_psrfits(fn, host_spectra(obs, palfa_synth()), obs)
    job = DedispJob([fn], resultsdir=str(tmp_path), tmpdir_base=str(tmp_path), device=0, backend="pdev",
                    workdir=str(tmp_path))
    d = copy.copy(job.ddplans[0])
    d.numpasses = 1
    job.ddplans = [d]
    try:
        with pytest.raises(PrestoError):
            run_pass(job, d, 0, None, job.tempdir, accel=dict())            # needs fft
        results = []
        dmstrs = dedisperse_job(job, fft=dict(zaplist=None, baryv=0.0, write=True),
                                accel=dict(numharm=8, sigma=2.0, flo=2.0, results=results))
        assert job.lo_accelsearch_time > 0
        assert len(results) == 1 and results[0][0] == dmstrs
        packed = np.stack([np.fromfile(os.path.join(job.tempdir, "%s_DM%s.fft" % (job.basefilenm, s)), np.float32)
                           for s in dmstrs])
        ora, _ = AO.search(packed, packed.shape[1] * obs.dt, numharm=8, sigma=2.0, flo=2.0)
        want = AO.prune(ora)
        got = results[0][1]
        assert len(got) == len(want) and len(got) > 0
        for f in ("dm", "numharm", "r2"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["power"].view(np.uint32), want["power"].view(np.uint32))
    finally:
        job.close()
