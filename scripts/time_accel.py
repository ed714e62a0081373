"""Timing aid (GPU box): hd_accel_search (hd_accel.hip) on one full-size pass of the C2 beam's
first DDplan stage (76 DMs x numout = choose_N(2^22), numharm 16, sigma 2.0, flo 2.0), on the
spectra its stage 1 + stage 2 + realfft + zapbirds-free rednoise leave in HBM.  After a
warm-up search: device ms of the two kernels (hipEvents, hd_accel_last_ms), wall ms of the
whole call (with the hit copy, sort and sigmas), the hit count, and the power plane's bytes."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pipeline2.0_amd")]
from hipdedisp import Engine, Opts, PassParams, plan as P  # noqa: E402
from hipdedisp import accel_stage as AS  # noqa: E402
from hipdedisp import fft_stage as FS  # noqa: E402
from hipdedisp.synth import palfa_obs, palfa_synth, rfifind_ptsperint, synth_mask  # noqa: E402

REPS = 5
obs = palfa_obs(N=1 << 22, nbits=8)
synth = palfa_synth()
with Engine(0) as eng:
    eng.set_obs(obs, Opts())
    eng.synth_device(synth)
    pts = rfifind_ptsperint(obs.dt)
    m, pad = synth_mask(obs, synth, pts)
    eng.set_mask(m, pts, pad)
    d = P.ddplans_for("pdev")[0]
    i = next(k for k in range(d.numpasses) if float(d.dmlist[k][0]) <= 71.0 <= float(d.dmlist[k][-1]))
    p = eng.plan(PassParams(subdm=float(d.subdmlist[i]), lodm=float(d.lodm_arg(i)), dmstep=float(d.dmstep_arg()),
                            numdms=d.dmsperpass, nsub=d.numsub, ds=d.sub_downsamp,
                            numout=P.choose_N(obs.N / d.downsamp)))
    p.run_subband()
    p.run_dedisp(to_host=False)
    T = p.numout * p.sub_dt
    FS.realfft(p)
    FS.rednoise(p, T)
    eng.sync()
    hits = AS.search(p, T, numharm=16, sigma=2.0, flo=2.0)      # warm-up (allocates the power plane)
    ms_p, ms_s, wall = [], [], []
    for _ in range(REPS):
        t = time.perf_counter()
        hits = AS.search(p, T, numharm=16, sigma=2.0, flo=2.0)
        wall.append(1e3 * (time.perf_counter() - t))
        a, b = AS.last_ms(p)
        ms_p.append(a)
        ms_s.append(b)
    kept = AS.prune(hits)
    gb = d.dmsperpass * p.numout * 4 / 1e9
    print("accel pass (%d DMs x numout %d, numharm 16, sigma 2.0): power plane %.3f ms, harmonic sums %.3f ms, "
          "device total %.3f ms (min of %d; medians %.3f + %.3f), call wall %.3f ms; %d hits, %d kept; "
          "P plane %.3f GB" % (d.dmsperpass, p.numout, min(ms_p), min(ms_s), min(x + y for x, y in zip(ms_p, ms_s)),
                               REPS, sorted(ms_p)[REPS // 2], sorted(ms_s)[REPS // 2], min(wall), len(hits), len(kept),
                               gb), flush=True)
    p.destroy()
