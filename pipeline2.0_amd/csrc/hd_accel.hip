// hd_accel.hip — the zero-acceleration harmonic-sum search of a pass's device-resident spectra:
// what the reference runs on every de-reddened .fft (lib/python/PALFA2_presto_search.py:560-568):
//     accelsearch -zmax 0 -numharm 16 -sigma 2.0 -flo 2.0 <fft>
// (lo_accel_*: lib/python/config/searching_example.py:20-23)
// [PRESTO-ext, parity with PRESTO unpinned: accelsearch is not in this image] restated so that
// tests/accel_oracle.py gives the power plane and the hits bit for bit from the same spectra:
//   * the spectrum F (numout/2 complex float32 bins after hd_rednoise, noise power about 1) is
//     read with F[0] and every bin outside [1, nb) taken as 0;
//   * half-bin power plane P[0 .. 2 nb): P[2k] = |F[k]|^2, P[2k+1] = the power of the Fourier
//     interpolation at k + 1/2 with kAccTaps taps a side, t_j = (float)(1 / (pi (j - 1/2))):
//     per component a float32 chain acc = acc + t_j * (F[k+j] - F[k+1-j]), j = 1 .. 16 in that
//     order, every operation rounded to float32 (no fused multiply-adds); the powers are
//     (float)((double)re^2 + (double)im^2); P[0] = P[1] = 0;
//   * harmonic sums at r2 (the top harmonic's frequency in half bins), stages H = 1, 2, 4, 8,
//     16: fraction m/16 of r2 lies at (r2 m + 8) >> 4 (= floor((2 r2 h + H) / (2 H)) for
//     h/H = m/16); a float32 add chain S = P[r2], + 1/2, + 1/4 + 3/4, + the odd eighths, + the
//     odd sixteenths, ascending; the value after each stage is that stage's summed power;
//   * per (DM, H) and aligned block of 64 half bins the largest S > (float)powcut_H with r2 in
//     [2 rlo, 2 rhi] is a hit (ties: the lowest r2); powcut_H is where the survival function
//     of a sum of H unit-mean exponentials, e^-P sum_{k<H} P^k / k!, times numindep_H =
//     (rhi - rlo) / H equals the normal tail beyond sigma.
// Not here: -zmax 50 (the f-dot plane), candidate optimisation and -harmpolish, accelsearch's
// own block-median normalisation, the _ACCEL_0 / .cand / .txtcand files, and sifting.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hd_internal.h"

#pragma clang fp contract(off)

namespace hd {

constexpr int kAccTaps = 16;      // interpolation taps a side
constexpr int kAccTile = 256;     // bins per k_acc_powers workgroup

struct AccTaps {
    float t[kAccTaps];
};
struct AccCuts {
    float cut[5];
};

// Tile of kAccTile bins of series blockIdx.y: the window F[k0 - 15 .. k0 + kAccTile + 16] in
// LDS (zero outside [1, nb)), then each thread forms its bin's two powers serially in the
// prescribed order and stores them as one float2 at P[2k].
__global__ __launch_bounds__(kAccTile) void k_acc_powers(const float2* __restrict__ F, int64_t fstride, int nb,
                                                         AccTaps taps, float* __restrict__ P, int64_t pstride)
{
    __shared__ float2 w[kAccTile + 2 * kAccTaps];
    const int k0 = blockIdx.x * kAccTile;
    const float2* f = F + (int64_t)blockIdx.y * fstride;
    for (int i = threadIdx.x; i < kAccTile + 2 * kAccTaps - 1; i += kAccTile) {
        const int b = k0 - (kAccTaps - 1) + i;
        w[i] = (b >= 1 && b < nb) ? f[b] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const int k = k0 + (int)threadIdx.x;
    if (k >= nb) return;
    const int c = (int)threadIdx.x + kAccTaps - 1;           // w[c] = F[k]
    const float2 z = w[c];
    float pe = (float)((double)z.x * (double)z.x + (double)z.y * (double)z.y);
    float I = 0.0f, Q = 0.0f;
#pragma unroll
    for (int j = 1; j <= kAccTaps; j++) {
        const float2 a = w[c + j], b = w[c + 1 - j];
        const float dx = a.x - b.x, dy = a.y - b.y;
        const float mx = taps.t[j - 1] * dx, my = taps.t[j - 1] * dy;
        I = I + mx;
        Q = Q + my;
    }
    float po = (float)((double)I * (double)I + (double)Q * (double)Q);
    if (k == 0) pe = po = 0.0f;
    *(float2*)(P + (int64_t)blockIdx.y * pstride + 2 * (int64_t)k) = make_float2(pe, po);
}

// One wave per aligned block of 64 half bins of series blockIdx.y (4 per workgroup): each lane
// its r2's five running sums from the 16 fractional positions of P, then per stage the wave's
// largest sum above the stage's threshold (the lowest lane among equals) appended through one
// counter.  Hits past cap are counted, not stored.
__global__ __launch_bounds__(256) void k_acc_harm(const float* __restrict__ P, int64_t pstride, int64_t r2lo,
                                                  int64_t r2hi, int nstage, AccCuts cuts,
                                                  hd_acc_hit* __restrict__ hits, unsigned long long* __restrict__ count,
                                                  int64_t cap)
{
    const int lane = threadIdx.x & 63;
    const int64_t blk = (r2lo >> 6) + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk * 64 > r2hi) return;                             // the whole wave
    const int64_t r2 = blk * 64 + lane;
    const bool in = r2 >= r2lo && r2 <= r2hi;
    const float* p = P + (int64_t)blockIdx.y * pstride;
    float S[5];
    float s = 0.0f;
    if (in) s = p[r2];
    S[0] = s;
#pragma unroll
    for (int st = 1; st < 5; st++) {
        if (st < nstage && in) {
            const int step = 16 >> st;
#pragma unroll
            for (int m = step; m < 16; m += 2 * step) s = s + p[(r2 * m + 8) >> 4];
        }
        S[st] = s;
    }
#pragma unroll
    for (int st = 0; st < 5; st++) {
        if (st >= nstage) break;
        const float v = (in && S[st] > cuts.cut[st]) ? S[st] : -__builtin_inff();
        float mx = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const unsigned long long win = __ballot(v == mx && v > -__builtin_inff());
        if (win != 0 && lane == __ffsll((long long)win) - 1) {
            const unsigned long long i = atomicAdd(count, 1ull);
            if ((int64_t)i < cap) {
                hd_acc_hit h;
                h.dm = (int32_t)blockIdx.y;
                h.numharm = 1 << st;
                h.r2 = (int32_t)r2;
                h.power = v;
                h.sigma = 0.0;
                hits[i] = h;
            }
        }
    }
}

hipError_t launch_acc_powers(const float2* F, int64_t fstride, int64_t nb, int ndm, const float* taps16, float* P,
                             int64_t pstride, hipStream_t st)
{
    AccTaps t;
    for (int j = 0; j < kAccTaps; j++) t.t[j] = taps16[j];
    hipLaunchKernelGGL(k_acc_powers, dim3((unsigned)((nb + kAccTile - 1) / kAccTile), ndm), dim3(kAccTile), 0, st, F,
                       fstride, (int)nb, t, P, pstride);
    return hipGetLastError();
}

hipError_t launch_acc_harm(const float* P, int64_t pstride, int ndm, int64_t r2lo, int64_t r2hi, int nstage,
                           const float* cut5, hd_acc_hit* hits, unsigned long long* count, int64_t cap, hipStream_t st)
{
    AccCuts c;
    for (int i = 0; i < 5; i++) c.cut[i] = cut5[i];
    const int64_t nblk = (r2hi >> 6) - (r2lo >> 6) + 1;
    hipLaunchKernelGGL(k_acc_harm, dim3((unsigned)((nblk + 3) / 4), ndm), dim3(256), 0, st, P, pstride, r2lo, r2hi,
                       nstage, c, hits, count, cap);
    return hipGetLastError();
}

// ---- host side: taps, thresholds, significances, the closest-r merge ---------------------

void accel_taps(float* taps16)
{
    for (int j = 1; j <= kAccTaps; j++) taps16[j - 1] = (float)(1.0 / (M_PI * ((double)j - 0.5)));
}

// log of e^-P sum_{k<H} P^k / k!
static double acc_log_q(int H, double P)
{
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < H; k++) {
        term = term * P / (double)k;
        sum += term;
    }
    return -P + std::log(sum);
}

// log of the normal tail beyond x: erfc while it is a normal number, past that the Mills
// ratio's continued fraction 1 / (x + 1 / (x + 2 / (x + ...))) on the density
// (*hazard, may be NULL: density / tail = -d log sf / dx, the continued fraction itself)
static double acc_log_sf(double x, double* hazard = nullptr)
{
    if (x < 5.0) {
        const double sf = 0.5 * std::erfc(x / M_SQRT2);
        if (hazard) *hazard = std::exp(-0.5 * x * x) / std::sqrt(2.0 * M_PI) / sf;
        return std::log(sf);
    }
    double t = x;
    for (int n = x < 12.0 ? 200 : 60; n >= 1; n--) t = x + (double)n / t;
    if (hazard) *hazard = t;
    return -0.5 * x * x - 0.5 * std::log(2.0 * M_PI) - std::log(t);
}

double accel_powcut(double sigma, int H, double numindep)
{
    const double target = acc_log_sf(sigma) - std::log(numindep);
    if (!(target < 0.0)) return 0.0;
    double lo = 0.0, hi = 64.0;
    while (hi < 1e12 && acc_log_q(H, hi) > target) hi *= 2.0;
    for (int it = 0; it < 200; it++) {                       // log Q falls with P: bisection to the last bit
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (acc_log_q(H, mid) > target) lo = mid;
        else hi = mid;
    }
    return hi;
}

double accel_sigma(double power, int H, double numindep)
{
    if (!(power > 0.0) || !std::isfinite(power)) return 0.0;
    const double logp = std::min(0.0, acc_log_q(H, power) + std::log(numindep));
    if (!(logp < std::log(0.5))) return 0.0;
    // log sf is concave and falling: Newton's first step from 0 lands right of the root and the
    // later ones fall to it monotonically (a thousand hits cost a millisecond); bisection stays
    // as the fallback
    double x = 0.0;
    for (int it = 0; it < 100; it++) {
        double hz;
        const double f = acc_log_sf(x, &hz) - logp;
        const double dx = f / hz;
        x += dx;
        if (std::fabs(dx) <= 1e-14 * x) return x;
    }
    double lo = 0.0, hi = 8.0;
    while (hi < 1e12 && acc_log_sf(hi) > logp) hi *= 2.0;
    for (int it = 0; it < 200; it++) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (acc_log_sf(mid) > logp) lo = mid;
        else hi = mid;
    }
    return hi;
}

// Per DM, hits in descending sigma (then lower numharm, lower r2); one is kept unless a kept
// one's fundamental r2 / (2 numharm) lies within closest_r bins.  Kept hits go to the front,
// DMs ascending, each DM's in that order.
int64_t accel_prune(hd_acc_hit* hits, int64_t n, double closest_r)
{
    std::vector<hd_acc_hit> v(hits, hits + n);
    std::sort(v.begin(), v.end(), [](const hd_acc_hit& a, const hd_acc_hit& b) {
        if (a.dm != b.dm) return a.dm < b.dm;
        if (a.sigma != b.sigma) return a.sigma > b.sigma;
        if (a.numharm != b.numharm) return a.numharm < b.numharm;
        return a.r2 < b.r2;
    });
    int64_t out = 0, dm0 = 0;                                // hits[dm0 .. out): the current DM's kept
    for (int64_t i = 0; i < n; i++) {
        const hd_acc_hit& h = v[(size_t)i];
        if (i == 0 || h.dm != v[(size_t)i - 1].dm) dm0 = out;
        const double f = (double)h.r2 / (2.0 * (double)h.numharm);
        bool keep = true;
        for (int64_t k = dm0; k < out && keep; k++)
            keep = !(std::fabs((double)hits[k].r2 / (2.0 * (double)hits[k].numharm) - f) < closest_r);
        if (keep) hits[out++] = h;
    }
    return out;
}

void accel_sort(hd_acc_hit* hits, int64_t n)
{
    std::sort(hits, hits + n, [](const hd_acc_hit& a, const hd_acc_hit& b) {
        if (a.dm != b.dm) return a.dm < b.dm;
        if (a.numharm != b.numharm) return a.numharm < b.numharm;
        return a.r2 < b.r2;
    });
}

}  // namespace hd
