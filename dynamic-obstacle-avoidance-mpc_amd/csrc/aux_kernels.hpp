// aux_kernels.hpp -- the small kernels either side of the solve: obstacle look-ahead (a9), warm-start shift (a12),
// initial guess (a13), plant step (a14), ground-truth obstacle motion and a dense dump of the linearisation for tests.
// File:line citations are relative to the reference repository root.
#pragma once
#include "rti_kernel.hpp"

namespace mpc {

// Obstacle.predict_trajectory (visualization.py:62-79) for every obstacle of every instance, written straight into the
// parameter tensor P[B][N+1][n_obst][2] (parameterize_model, robot_ocp_problem.py:154-166).  One thread per obstacle.
__global__ void predict_kernel(World w, int count, int n_obst, int N, double dt, const double *__restrict__ obst, double *__restrict__ P)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int inst = t / n_obst, j = t - inst * n_obst;
    const double *o = obst + (size_t)t * 4;
    double x = o[0], y = o[1], vy = o[3];
    double vx = w.bug_compat_predict ? o[3] : o[2];   // visualization.py:69 (reference defect D1)
    double *Pi = P + ((size_t)inst * (N + 1) * n_obst + j) * 2;
    Pi[0] = x; Pi[1] = y;
    for (int i = 1; i <= N; i++) {
        obstacle_advance(w, dt, x, vx, y, vy);
        Pi[(size_t)i * n_obst * 2] = x; Pi[(size_t)i * n_obst * 2 + 1] = y;
    }
}

// Obstacle.step(): ground-truth motion with optional multiplicative velocity noise, visualization.py:20-33.
__global__ void obstacle_step_kernel(World w, int count, double dt, double *__restrict__ obst, const double *__restrict__ noise,
                                     double randomness, double vmax)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    double *o = obst + (size_t)t * 4;
    double x = o[0], y = o[1], vx = o[2], vy = o[3];
    if (noise) obstacle_noise(randomness, vmax, noise[(size_t)t * 2], noise[(size_t)t * 2 + 1], vx, vy);
    obstacle_advance(w, dt, x, vx, y, vy);
    o[0] = x; o[1] = y; o[2] = vx; o[3] = vy;
}

// generate_random_moving_obstacles (obstacle_generator.py:8-28) for `count` seeds: thread s reproduces what the reference draws
// after np.random.seed(seed0 + s) -- numpy's legacy MT19937 (init_genrand seeding, standard tempering), random_sample() =
// ((a >> 5) * 2^26 + (b >> 6)) / 2^53 from two consecutive outputs, uniform(lo, hi) = lo + (hi - lo) * u (no contraction), drawn in
// the reference's order: x block, y block (RANDOM only), vx block, vy block.  CENTER / EDGE place every obstacle at 0 / `edge`.
// At most 8 * n_obst <= 80 outputs are needed, all from the first state regeneration, which touches state words < 80 + 398.
enum { kScenarioRandom = 0, kScenarioCenter = 1, kScenarioEdge = 2 };
__global__ void scenario_kernel(int count, int n_obst, int scenario, unsigned seed0, double x_lo, double x_hi, double y_lo, double y_hi,
                                double v_max, double edge, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    constexpr int kWords = 80 + 398;
    unsigned mt[kWords];
    mt[0] = seed0 + (unsigned)s;
    for (int k = 1; k < kWords; k++) mt[k] = 1812433253u * (mt[k - 1] ^ (mt[k - 1] >> 30)) + (unsigned)k;
    int pos = 0;
    auto next32 = [&]() {
        const unsigned y0 = (mt[pos] & 0x80000000u) | (mt[pos + 1] & 0x7fffffffu);
        unsigned y = mt[pos + 397] ^ (y0 >> 1) ^ ((y0 & 1u) ? 0x9908b0dfu : 0u);
        pos++;
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    };
    auto uniform = [&](double lo, double hi) {
        const unsigned a = next32() >> 5, b = next32() >> 6;
        const double u = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
        return lo + (hi - lo) * u;
    };
    double *o = out + (size_t)s * n_obst * 4;
    for (int j = 0; j < n_obst; j++) o[j * 4 + 0] = scenario == kScenarioRandom ? uniform(x_lo, x_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 1] = scenario == kScenarioRandom ? uniform(y_lo, y_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 2] = uniform(-v_max, v_max);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 3] = uniform(-v_max, v_max);
}

// ------------------------------------------------------------------------------------------------------------------
// THE REFERENCE'S NOISE STREAM ON THE DEVICE.  experiments.py:33-36 seeds numpy's global legacy generator per run (np.random.seed(i)), draws the
// scenario (obstacle_generator.py: uniform blocks) and then, in every control step, `for o in self.obstacles: o.step()` draws np.random.normal(size=2)
// per obstacle (visualization.py:31).  Instance s of a batch carries that generator for seed seed0 + s: MT19937 state (624 words), position, and the
// cached second value of the polar Gaussian method -- numpy's legacy_gauss:
//     if cached: return it;  else  do { x1 = 2 u - 1; x2 = 2 u - 1; r2 = x1 x1 + x2 x2 } while (r2 >= 1 || r2 == 0);  f = sqrt(-2 log(r2) / r2);
//     cache f x1, return f x2                       (u = random_sample() = ((a >> 5) 2^26 + (b >> 6)) / 2^53 from two outputs)
// Everything but the logarithm is IEEE arithmetic in numpy's order (no contraction) and therefore bit-exact.  The logarithm is evaluated to ~2^-80 in
// double-double arithmetic and rounded once, i.e. correctly rounded for all practical purposes; glibc's log (what numpy calls) is not quite -- it
// differs from the correctly rounded value on a few inputs in 10^5 -- so the stream equals the host's in all but that fraction of the draws, where
// one value differs in its last bit (measured: tests/test_gpu_aux.py).  The device library's own log differs from glibc's on 2.8 % of the inputs.
// State layout per instance (uint32 words): mt[624] | pos | has_gauss | gauss (2 words).
constexpr int kNoiseStateWords = 628;

__device__ __forceinline__ void dd_two_sum(double a, double b, double &s, double &e)
{
#pragma clang fp contract(off)
    s = a + b; const double bb = s - a; e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void dd_fast_two_sum(double a, double b, double &s, double &e)       // |a| >= |b|
{
#pragma clang fp contract(off)
    s = a + b; e = b - (s - a);
}
// (ah, al) * (bh, bl) -> (ph, pl), error ~2^-104
__device__ __forceinline__ void dd_mul(double ah, double al, double bh, double bl, double &ph, double &pl)
{
    ph = ah * bh;
    pl = fma(ah, bh, -ph) + (ah * bl + al * bh);
    double s, e; dd_fast_two_sum(ph, pl, s, e); ph = s; pl = e;
}
__device__ __forceinline__ void dd_add(double ah, double al, double bh, double bl, double &sh, double &sl)
{
    double s, e; dd_two_sum(ah, bh, s, e);
    e += al + bl;
    dd_fast_two_sum(s, e, sh, sl);
}
// log(x) for a normal positive double, rounded once from a double-double value
__device__ inline double log_dd(double x)
{
    static constexpr double kLogTab[25][2] = {{-0x1.7fafa3bd8151cp-2, 0x1.219024acd3b77p-58}, {-0x1.522ae0738a3d8p-2, 0x1.8f7e9b38a6979p-57}, {-0x1.269621134db92p-2, -0x1.e0efadd9db02bp-56}, {-0x1.f991c6cb3b379p-3, -0x1.f665066f980a2p-57}, {-0x1.a93ed3c8ad9e3p-3, -0x1.bcafa9de97203p-57}, {-0x1.5bf406b543db2p-3, 0x1.1f5b44c0df7e7p-61}, {-0x1.1178e8227e47cp-3, 0x1.0e63a5f01c691p-58}, {-0x1.9335e5d594989p-4, 0x1.478a85704ccb7p-58}, {-0x1.08598b59e3a07p-4, 0x1.dd7009902bf32p-58}, {-0x1.0415d89e74444p-5, -0x1.c05cf1d753622p-59}, {0x0.0p+0, 0x0.0p+0}, {0x1.f829b0e783300p-6, 0x1.33e3f04f1ef23p-60}, {0x1.f0a30c01162a6p-5, 0x1.85f325c5bbacdp-59}, {0x1.6f0d28ae56b4cp-4, -0x1.906d99184b992p-58}, {0x1.e27076e2af2e6p-4, -0x1.61578001e0162p-60}, {0x1.29552f81ff523p-3, 0x1.301771c407dbfp-57}, {0x1.5ff3070a793d4p-3, -0x1.bc60efafc6f6ep-58}, {0x1.9525a9cf456b4p-3, 0x1.d904c1d4e2e26p-57}, {0x1.c8ff7c79a9a22p-3, -0x1.4f689f8434012p-57}, {0x1.fb9186d5e3e2bp-3, -0x1.caaae64f21acbp-57}, {0x1.1675cababa60ep-2, 0x1.ce63eab883717p-61}, {0x1.2e8e2bae11d31p-2, -0x1.8f4cdb95ebdf9p-56}, {0x1.4618bc21c5ec2p-2, 0x1.f42decdeccf1dp-56}, {0x1.5d1bdbf5809cap-2, 0x1.4236383dc7fe1p-56}, {0x1.739d7f6bbd007p-2, -0x1.8c76ceb014b04p-56}};
    int e;
    double m = frexp(x, &e);                        // m in [0.5, 1)
    if (m < 0.70710678118654752) { m *= 2.0; e -= 1; }      // m in [sqrt(1/2), sqrt(2)): log x = e ln 2 + log m without cancellation near x = 1
    const int i = (int)rint(m * 32.0);              // 22 .. 46; c = i / 32 exactly, |m - c| <= 1 / 64
    const double c = (double)i * 0.03125;
    // t = (m - c) / (m + c) in double-double: the numerator is exact (m and c within a factor of two: Sterbenz)
    const double num = m - c;
    double dh, dl; dd_two_sum(m, c, dh, dl);
    const double th = num / dh;
    const double tl = (fma(-th, dh, num) - th * dl) / dh;
    // log m = log c + 2 atanh t = log c + 2 (t + t^3 / 3 + t^5 / 5 + ...): t and t^3 / 3 in double-double, the rest (<= 3e-9 t) in double
    double t2h, t2l; dd_mul(th, tl, th, tl, t2h, t2l);
    double t3h, t3l; dd_mul(t2h, t2l, th, tl, t3h, t3l);
    double ch, cl; dd_mul(t3h, t3l, 0x1.5555555555555p-2, 0x1.5555555555555p-56, ch, cl);
    const double w = t2h;
    const double tail = th * (w * w) * (1.0 / 5.0 + w * (1.0 / 7.0 + w * (1.0 / 9.0 + w * (1.0 / 11.0 + w * (1.0 / 13.0)))));
    double ah, al; dd_add(th, tl, ch, cl, ah, al);
    al += tail;
    ah *= 2.0; al *= 2.0;
    double rh, rl; dd_add(kLogTab[i - 22][0], kLogTab[i - 22][1], ah, al, rh, rl);
    // e ln 2: the high part of ln 2 has 11 trailing zero bits, so e * ln2_hi is exact
    const double ed = (double)e;
    double eh = ed * 0x1.62e42fefa3800p-1, el = ed * 0x1.ef35793c76730p-45 + ed * 0x1.f97b57a079a19p-103;
    double sh, sl; dd_add(eh, el, rh, rl, sh, sl);
    return sh + sl;
}

struct NoiseGen {
    unsigned *st;      // this instance's state words
    __device__ __forceinline__ unsigned next32()
    {
        int pos = (int)st[624];
        if (pos >= 624) {       // regenerate (numpy's rk_random / init by genrand: the standard twist)
            for (int k = 0; k < 624; k++) {
                const unsigned y0 = (st[k] & 0x80000000u) | (st[(k + 1) % 624] & 0x7fffffffu);
                st[k] = st[(k + 397) % 624] ^ (y0 >> 1) ^ ((y0 & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        unsigned y = st[pos];
        st[624] = (unsigned)(pos + 1);
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
    __device__ __forceinline__ double next_double()
    {
#pragma clang fp contract(off)
        const unsigned a = next32() >> 5, b = next32() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
    __device__ __forceinline__ double gauss()
    {
#pragma clang fp contract(off)
        if (st[625]) {
            st[625] = 0u;
            const double g = __hiloint2double((int)st[627], (int)st[626]);
            st[626] = 0u; st[627] = 0u;
            return g;
        }
        double x1, x2, r2;
        do {
            x1 = 2.0 * next_double() - 1.0;
            x2 = 2.0 * next_double() - 1.0;
            const double a = x1 * x1, b = x2 * x2;
            r2 = a + b;
        } while (r2 >= 1.0 || r2 == 0.0);
        const double lg = log_dd(r2);
        const double q = -2.0 * lg;
        const double f = sqrt(q / r2);
        const double g = f * x1;
        st[625] = 1u; st[626] = (unsigned)__double2loint(g); st[627] = (unsigned)__double2hiint(g);
        return f * x2;
    }
};

// np.random.seed(seed0 + s) followed by the scenario generator's uniform draws (their VALUES come from scenario_kernel; here they are only consumed):
// 4 n_obst doubles for RANDOM (x, y, vx, vy blocks), 2 n_obst otherwise
__global__ void noise_init_kernel(int count, int n_obst, int scenario, unsigned seed0, unsigned *__restrict__ state)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    unsigned *st = state + (size_t)s * kNoiseStateWords;
    st[0] = seed0 + (unsigned)s;
    for (int k = 1; k < 624; k++) st[k] = 1812433253u * (st[k - 1] ^ (st[k - 1] >> 30)) + (unsigned)k;
    st[624] = 624u; st[625] = 0u; st[626] = 0u; st[627] = 0u;
    NoiseGen g{st};
    const int draws = (scenario == kScenarioRandom ? 4 : 2) * n_obst;
    for (int k = 0; k < draws; k++) (void)g.next_double();
}

// scenario_kernel for more than 10 obstacles: 8 n_obst > 227 outputs reach past the words the first regeneration can take from the seeded state, so the
// whole MT19937 state is kept (NoiseGen, private memory) and regenerated in place -- the same draws, the same values
__global__ void scenario_wide_kernel(int count, int n_obst, int scenario, unsigned seed0, double x_lo, double x_hi, double y_lo, double y_hi,
                                     double v_max, double edge, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    unsigned st[kNoiseStateWords];
    st[0] = seed0 + (unsigned)s;
    for (int k = 1; k < 624; k++) st[k] = 1812433253u * (st[k - 1] ^ (st[k - 1] >> 30)) + (unsigned)k;
    st[624] = 624u; st[625] = 0u; st[626] = 0u; st[627] = 0u;
    NoiseGen g{st};
    auto uniform = [&](double lo, double hi) { const double u = g.next_double(); return lo + (hi - lo) * u; };
    double *o = out + (size_t)s * n_obst * 4;
    for (int j = 0; j < n_obst; j++) o[j * 4 + 0] = scenario == kScenarioRandom ? uniform(x_lo, x_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 1] = scenario == kScenarioRandom ? uniform(y_lo, y_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 2] = uniform(-v_max, v_max);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 3] = uniform(-v_max, v_max);
}

// one control step's np.random.normal(size=2) per obstacle, in the reference's order (obstacle 0 first): noise[s][j][0..1]
__global__ void noise_draw_kernel(int count, int n_obst, unsigned *__restrict__ state, double *__restrict__ noise, const int32_t *__restrict__ ep_flags)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    if (ep_flags && (ep_flags[s] & 1)) return;      // the episode is over: the reference's loop has left (robot_ocp_problem.py:247-250), nothing is drawn any more
    NoiseGen g{state + (size_t)s * kNoiseStateWords};
    double *o = noise + (size_t)s * n_obst * 2;
    for (int j = 0; j < n_obst; j++) { o[2 * j] = g.gauss(); o[2 * j + 1] = g.gauss(); }
}

// INSTANCE SCHEDULING.  Where several instances share a wavefront (one lane per stage: 2, 3 or 4 of them) the wavefront runs until its
// slowest instance has converged, and interior-point iteration counts are heavy-tailed: on the randomized C3 workload the mean is 6.6 but the
// mean of the per-wavefront maximum is 8.2 with two and 9.4 with three instances per wavefront.  Iteration counts of consecutive control
// steps of one instance are strongly correlated, so dealing the instances to wavefronts IN THE ORDER OF THEIR PREVIOUS COUNT brings the
// per-wavefront maximum down to 7.1 / 7.4 (scripts/iters_order_probe.py).  These kernels build that order: a stable counting sort of the
// instances by their last iteration count, descending (the longest-running wavefronts are dispatched first): deterministic, O(batch),
// ~10 us at 65536.
// order[] is a permutation of 0..batch-1; the solve kernel's slot s processes instance order[s].  Results are those of the natural
// order (bit for bit with 2 or 4 instances per wavefront; to the rounding of the wavefront sums with 3).
// Two launches: schedule_count_kernel (one histogram per block of kSchedChunk consecutive instances) and schedule_scatter_kernel (every block
// derives its global base per bin from all histograms, ranks its own instances stably and writes their slots).
constexpr int kSchedThreads = 256, kSchedBins = 32, kSchedPer = 4, kSchedChunk = kSchedThreads * kSchedPer;   // counts >= 31 share the first bin
__device__ __forceinline__ int sched_key(int it) { return (kSchedBins - 1) - (it < 0 ? 0 : (it > kSchedBins - 1 ? kSchedBins - 1 : it)); }   // descending counts

__global__ __launch_bounds__(kSchedThreads) void schedule_count_kernel(int batch, int nblk, const int32_t *__restrict__ iters, unsigned *__restrict__ ghist)
{
    __shared__ unsigned hist[kSchedBins];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < kSchedBins) hist[t] = 0u;
    __syncthreads();
    const int e0 = b * kSchedChunk + t * kSchedPer;
#pragma unroll
    for (int u = 0; u < kSchedPer; u++)
        if (e0 + u < batch) __hip_atomic_fetch_add(&hist[sched_key(iters[e0 + u])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (t < kSchedBins) ghist[t * nblk + b] = hist[t];          // bin-major: the scatter pass reads a bin's blocks consecutively
}

__global__ __launch_bounds__(kSchedThreads) void schedule_scatter_kernel(int batch, int nblk, const int32_t *__restrict__ iters,
                                                                         const unsigned *__restrict__ ghist, int32_t *__restrict__ order)
{
    __shared__ unsigned cnt[kSchedBins * kSchedThreads];      // [bin][thread]: counts, then exclusive offsets in (bin, thread) order
    __shared__ unsigned part[kSchedThreads], tot[kSchedBins], pre[kSchedBins], base[kSchedBins], row0[kSchedBins];
    const int t = threadIdx.x, b = blockIdx.x;
    for (int f = t; f < kSchedBins * kSchedThreads; f += kSchedThreads) cnt[f] = 0u;
    if (t < kSchedBins) { tot[t] = 0u; pre[t] = 0u; }
    __syncthreads();
    // (a) where this block's instances of every bin start: everything in earlier bins, plus the same bin in earlier blocks
    for (int f = t; f < kSchedBins * nblk; f += kSchedThreads) {
        const int bin = f / nblk, blk = f - bin * nblk;
        const unsigned v = ghist[f];
        if (v) {
            __hip_atomic_fetch_add(&tot[bin], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (blk < b) __hip_atomic_fetch_add(&pre[bin], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    // (b) this block's own instances: thread t owns kSchedPer consecutive ones, counted in column t
    const int e0 = b * kSchedChunk + t * kSchedPer;
    int key[kSchedPer];
#pragma unroll
    for (int u = 0; u < kSchedPer; u++) {
        key[u] = (e0 + u < batch) ? sched_key(iters[e0 + u]) : -1;
        if (key[u] >= 0) cnt[key[u] * kSchedThreads + t] += 1u;
    }
    __syncthreads();
    if (t == 0) { unsigned run = 0u; for (int k = 0; k < kSchedBins; k++) { base[k] = run + pre[k]; run += tot[k]; } }
    // exclusive scan of cnt in (bin, thread) order: thread t owns the kSchedBins consecutive entries [t * kSchedBins, (t + 1) * kSchedBins)
    unsigned sum = 0u;
    for (int f = 0; f < kSchedBins; f++) sum += cnt[t * kSchedBins + f];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kSchedThreads; d <<= 1) {
        const unsigned v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned run = part[t] - sum;
    for (int f = 0; f < kSchedBins; f++) { const unsigned c = cnt[t * kSchedBins + f]; cnt[t * kSchedBins + f] = run; run += c; }
    __syncthreads();
    if (t < kSchedBins) row0[t] = cnt[t * kSchedThreads];     // offset of the bin's first instance inside this block
    __syncthreads();
    // (c) slots: bins in descending-count order, inside a bin ascending instance index (blocks, threads, a thread's own instances in order)
#pragma unroll
    for (int u = 0; u < kSchedPer; u++) {
        if (key[u] >= 0) {
            const int k = key[u] * kSchedThreads + t;
            order[base[key[u]] + (cnt[k] - row0[key[u]])] = e0 + u;
            cnt[k] += 1u;
        }
    }
}

// Warm-start shift, robot_ocp_problem.py:253-258: X[j] <- X[j+1] (j < N), U[j] <- U[j+1] (j < N-1), U[N-1] <- 0.
// One wavefront per instance; every lane reads its successor stage before anyone writes.
__global__ __launch_bounds__(64) void shift_kernel(int batch, int N, double *__restrict__ X, double *__restrict__ U)
{
    const int inst = blockIdx.x;
    if (inst >= batch) return;
    const int i = threadIdx.x;
    double *Xg = X + (size_t)inst * (N + 1) * 5, *Ug = U + (size_t)inst * N * 2;
    double xv[5] = {0, 0, 0, 0, 0}, uv[2] = {0, 0};
    if (i < N) {
#pragma unroll
        for (int c = 0; c < 5; c++) xv[c] = Xg[(i + 1) * 5 + c];
    }
    if (i < N - 1) { uv[0] = Ug[(i + 1) * 2]; uv[1] = Ug[(i + 1) * 2 + 1]; }
    __syncthreads();
    if (i < N) {
#pragma unroll
        for (int c = 0; c < 5; c++) Xg[i * 5 + c] = xv[c];
        Ug[i * 2] = uv[0]; Ug[i * 2 + 1] = uv[1];
    }
}

// set_initial_guess, robot_ocp_problem.py:286-306: X[i] = [x0_x, x0_y, x0_psi, 0, 0], U = 0.
// goal != null: the straight-line variant of the commented block :293-300 (interp_guess, rti_kernel.hpp).
__global__ void reset_guess_kernel(int batch, int N, const double *__restrict__ x0, const double *__restrict__ goal, double *__restrict__ X, double *__restrict__ U)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= batch * (N + 1)) return;
    const int inst = t / (N + 1), i = t - inst * (N + 1);
    const double *x = x0 + (size_t)inst * 5;
    double *Xi = X + (size_t)t * 5;
    Xi[0] = x[0]; Xi[1] = x[1]; Xi[2] = x[2]; Xi[3] = 0.0; Xi[4] = 0.0;
    if (goal) {
        const double xs[5] = {x[0], x[1], x[2], x[3], x[4]};
        double xg[5];
        interp_guess(xs, goal[(size_t)inst * 2 + 1], i, N, xg);
#pragma unroll
        for (int c = 0; c < 5; c++) Xi[c] = xg[c];
    }
    if (i < N) { double *Ui = U + ((size_t)inst * N + i) * 2; Ui[0] = 0.0; Ui[1] = 0.0; }
}

// MULTI-START (mpc_seed_guesses_dev, mpc_select_best_dev): a batch of `groups` scenarios with K candidate iterates each -- member k of group g is instance
// g K + k, and every member of a group is given the same x0, obstacles and goal.  The solve between the two launches is the ordinary one on groups * K
// instances; these two kernels stand beside it.  (No reference counterpart: robot_ocp_problem.py:286-306 starts every solve from one guess.)
//
// seed_guesses_kernel: the iterate of member k is the straight line from x0 to the goal bent sideways by a half sine of amplitude a = offsets[k] metres --
// with d = goal - x0[0:2], L = |d|, t = d / L, n = (-t_y, t_x), s_i = i / N:
//   position  X[i][0:2] = x0[0:2] + s_i d + a sin(pi s_i) n,
//   heading   X[i][2]   = psi0 + wrap(atan2(tau_y, tau_x) - psi0) along the path tangent tau = d + a pi cos(pi s_i) n, wrap(e) = e - 2 pi rint(e / 2 pi)
//             (the heading nearest to psi0 modulo a turn: an unwrapped jump of 2 pi would be a spin in the model),
//   X[i][3:5] = 0 for i >= 1, X[0] = x0 (all five), U = 0.
// L < 1e-9: the plain guess of reset_guess_kernel (a robot on its goal has no direction to bend).  keep_first: member 0 of every group is left alone (the
// closed loop's shifted warm start).  Non-finite inputs propagate into the iterate; the solve then reports status 4 as for any such warm start.
// One wavefront per instance, a stage per lane (N + 1 <= 63), four instances per workgroup; every word written belongs to the wavefront's own instance.
constexpr int kGroupThreads = 256, kGroupWaves = kGroupThreads / 64;
constexpr double kPi = 3.14159265358979323846;

// stage i of the family's iterate with offset a around the state x and d = goal - x[0:2] of length L, written ONCE for seed_guesses_kernel and
// group_step_kernel: s = i / N, sn = sin(pi s), cs = cos(pi s) are the caller's (a lane forms them once for all the members it writes)
__device__ __forceinline__ void seed_stage(const double x[5], double dx, double dy, double L, double a, int i, double s, double sn, double cs, double xi[5])
{
    const double px = x[0], py = x[1], psi = x[2];
    xi[0] = px; xi[1] = py; xi[2] = psi; xi[3] = 0.0; xi[4] = 0.0;
    if (!(L < 1e-9)) {                                          // (a NaN length takes this branch and propagates)
        if (i == 0) {
            xi[3] = x[3]; xi[4] = x[4];
        } else {
            const double nx = -dy / L, ny = dx / L;
            xi[0] = px + s * dx + a * sn * nx;
            xi[1] = py + s * dy + a * sn * ny;
            const double e = atan2(dy + a * kPi * cs * ny, dx + a * kPi * cs * nx) - psi;
            xi[2] = psi + (e - 2.0 * kPi * rint(e / (2.0 * kPi)));
        }
    }
}

// a lane's obstacle row, row `row` of an [..][4] array, written ONCE for the group kernels (geometry seed, group step, group refill).  The kernels that
// fence their loads (group_step_kernel, group_refill_apply_kernel) load above the fence and store behind it; the pair holds no rule.  (The stage store, the
// lane pick and the member-input store of these kernels stay written out: as helpers of any shape tried they changed the kernels' instructions.)
__device__ __forceinline__ void load_obst_row(const double *obst, size_t row, double ob[4])
{
    const double *o = obst + row * 4;
    ob[0] = o[0]; ob[1] = o[1]; ob[2] = o[2]; ob[3] = o[3];
}
__device__ __forceinline__ void store_obst_row(double *obst, size_t row, const double ob[4])
{
    double *o = obst + row * 4;
    o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2]; o[3] = ob[3];
}

__global__ __launch_bounds__(kGroupThreads) void seed_guesses_kernel(int groups, int K, int N, int keep_first, const double *__restrict__ x0,
                                                                     const double *__restrict__ goal, const double *__restrict__ offsets,
                                                                     double *__restrict__ X, double *__restrict__ U)
{
    const int i = threadIdx.x & 63;
    const int inst = blockIdx.x * kGroupWaves + (threadIdx.x >> 6);
    if (inst >= groups * K) return;
    const int g = inst / K, k = inst - g * K;
    if ((keep_first && k == 0) || i > N) return;
    const double x[5] = {x0[(size_t)g * 5], x0[(size_t)g * 5 + 1], x0[(size_t)g * 5 + 2], x0[(size_t)g * 5 + 3], x0[(size_t)g * 5 + 4]};
    const double dx = goal[(size_t)g * 2] - x[0], dy = goal[(size_t)g * 2 + 1] - x[1];
    const double L = sqrt(dx * dx + dy * dy);
    const double s = (double)i / (double)N;
    double xi[5];
    seed_stage(x, dx, dy, L, offsets[k], i, s, sin(kPi * s), cos(kPi * s), xi);
    double *Xi = X + ((size_t)inst * (N + 1) + i) * 5;
#pragma unroll
    for (int c = 0; c < 5; c++) Xi[c] = xi[c];
    if (i < N) { double *Ui = U + ((size_t)inst * N + i) * 2; Ui[0] = 0.0; Ui[1] = 0.0; }
}

// select_best_kernel: per group, the eligible member (status 0 or 2, finite cost) of least cost, ties to the lowest member index; with margin m > 0 an
// eligible member 0 stays the winner unless the challenger costs less than (1 - m) cost[0] (hysteresis: the closed loop keeps member 0 = the shifted
// winner of the last step).  No eligible member: winner -1, best_cost +inf, best_u0 (0, 0), nothing copied.
// One wavefront per group, four groups per workgroup.  Lane k < K holds (cost, k); lanes without an eligible member hold (+inf, 64 + lane), which sorts
// behind every eligible pair.  The argmin is a butterfly of six cross-lane exchanges (distances 32 .. 1) with a lexicographic compare -- min is associative and
// commutative on a total order, so every lane ends with the same pair whatever the order: no atomics, no dependence on which workgroup runs when.
// kSelectBroadcast: the winner's row of X (5 (N + 1) doubles) and of U (2 N) is read ONCE into registers, the lanes striding over it (consecutive lanes,
// consecutive doubles: 512 contiguous bytes per load), and stored to the K - 1 other rows of the group the same way -- never onto itself, so no word is
// both read and written in one launch.  Row lengths need not be multiples of 64: the last round is partly masked.
constexpr int kSelectBroadcast = 1;                             // MPC_SELECT_BROADCAST
constexpr int kSelectXRounds = 5, kSelectURounds = 2;           // 64 x 5 >= 5 (N + 1), 64 x 2 >= 2 N for N <= 62

// the rule itself, written ONCE for select_best_kernel and group_step_kernel: called by all 64 lanes of the group's wavefront, every lane returns the
// winner (-1: no eligible member) and gets its cost in c (+inf without a winner)
__device__ __forceinline__ int select_member(int K, double margin, const double *__restrict__ cost, const int32_t *__restrict__ status, size_t base,
                                             int lane, double &c)
{
    c = INFINITY;
    int idx = 64 + lane;
    if (lane < K) {
        const double cc = cost[base + lane];
        const int st = status[base + lane];
        if ((st == 0 || st == 2) && isfinite(cc)) { c = cc; idx = lane; }
    }
    const double c0 = __shfl(c, 0);
    const bool keep0 = __shfl(idx, 0) == 0;                     // member 0 is eligible
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oc = __shfl_xor(c, m);
        const int oi = __shfl_xor(idx, m);
        if (oc < c || (oc == c && oi < idx)) { c = oc; idx = oi; }
    }
    if (margin > 0.0 && keep0 && idx != 0 && !(c < (1.0 - margin) * c0)) { c = c0; idx = 0; }
    if (idx >= 64) c = INFINITY;
    return idx < 64 ? idx : -1;
}

// GUESS FAMILY FROM GEOMETRY (mpc_set_guess_geometry; include/mpc_gpu.h states the rule): the amplitudes of one group's members from the obstacles in the
// way, written ONCE for seed_guesses_geom_kernel, group_step_kernel<true> and group_refill_apply_kernel<true>.  Called by all 64 lanes of a wavefront that
// holds one group: (px, py) and (gx, gy) are the group's (the same on every lane), lane j < no holds obstacle j in ob, its radius r and its mask bit in
// `present`, lane k < K holds offsets[k] in base; lane k returns the amplitude of member k (lanes >= K: base).  The rank of a blocking obstacle is a
// count over the no obstacle lanes with the lexicographic compare (al, j); the member lanes then look for rank (k - 1) >> 1 and fetch its left / right.
// The loops run to the run-time count `no` (wave-uniform) and no cross-lane step stands under a lane-dependent branch; no LDS, no atomics.  Contraction
// is off so that the three callers and a host restatement round the same operations.
struct GuessGeom { int mode; double clearance, a_max, lead, r_safe; const double *ip_r2; const uint32_t *omask; };

// the radius and the mask bit the rule reads for obstacle `lane` of the group whose first member is instance `base`: row `base` of the per-instance
// tables where the handle has them.  The table holds r_safe^2 (KParams::ip_r2), and sqrt(fl(r r)) = r in binary64 for any r whose square neither
// overflows nor underflows (radii are finite and > 0), so the root is the caller's r_safe bit for bit
__device__ __forceinline__ void guess_geometry_row(const GuessGeom &q, size_t base, int no, int lane, double &r, bool &present)
{
    r = q.r_safe; present = lane < no;
    if (lane < no) {
        if (q.ip_r2) r = sqrt(q.ip_r2[base * no + lane]);
        if (q.omask) present = (omask_word(q.omask, (int)base, no) >> lane) & 1u;
    }
}

__device__ __forceinline__ double guess_amplitudes(const GuessGeom &q, int K, int no, int lane, double px, double py, double gx, double gy,
                                                   const double ob[4], double r, bool present, double base)
{
#pragma clang fp contract(off)
    const double dx = gx - px, dy = gy - py;
    const double L = sqrt(dx * dx + dy * dy);
    const double tx = dx / L, ty = dy / L;
    const double qx = ob[0] + q.lead * ob[2], qy = ob[1] + q.lead * ob[3];
    const double ex = qx - px, ey = qy - py;
    const double al = ex * tx + ey * ty, c = ex * (-ty) + ey * tx;
    const double s = al / L, R = r + q.clearance;
    const bool blocks = lane < no && present && s > 0.0 && s < 1.0 && fabs(c) < R;       // (a NaN fails every compare)
    const double w = sin(kPi * s);
    const double left = fmin(fmax((c + R) / w, -q.a_max), q.a_max), right = fmin(fmax((c - R) / w, -q.a_max), q.a_max);
    int rank = blocks ? 0 : -1;
    for (int j = 0; j < no; j++) {
        const double aj = __shfl(al, j);
        const int bj = __shfl((int)blocks, j);
        if (blocks && bj && (aj < al || (aj == al && j < lane))) rank++;
    }
    const int want = lane >= 1 && lane < K ? (lane - 1) >> 1 : -2;
    int src = -1;
    for (int j = 0; j < no; j++)
        if (__shfl(rank, j) == want) src = j;
    const double lj = __shfl(left, src < 0 ? 0 : src), rj = __shfl(right, src < 0 ? 0 : src);
    double amp = base;
    if (src >= 0 && !(L < 1e-9)) amp = (lane & 1) ? lj : rj;
    return amp;
}

// seed_guesses_kernel with the amplitudes from the geometry (mpc_seed_guesses_geom_dev): the same layout -- one wavefront per instance, a stage per lane,
// four instances per workgroup -- and each wavefront evaluates its GROUP's rule for itself (obstacle j of the group on lane j, the base family on the
// member lanes) and reads out its own member's amplitude; the wavefront of member 0 also stores the group's K amplitudes into offsets_out.  No lane
// leaves in front of the cross-lane steps.  Every word written belongs to the wavefront's own instance (offsets_out: to its own group, by member 0).
__global__ __launch_bounds__(kGroupThreads) void seed_guesses_geom_kernel(GuessGeom q, int groups, int K, int N, int n_obst, int keep_first,
                                                                          const double *__restrict__ x0, const double *__restrict__ obst,
                                                                          const double *__restrict__ goal, const double *__restrict__ offsets,
                                                                          double *__restrict__ X, double *__restrict__ U, double *__restrict__ offsets_out)
{
    const int i = threadIdx.x & 63;
    const int inst = __builtin_amdgcn_readfirstlane(blockIdx.x * kGroupWaves + (threadIdx.x >> 6));
    if (inst >= groups * K) return;                             // (wave-uniform)
    const int g = inst / K, k = inst - g * K;
    const double x[5] = {x0[(size_t)g * 5], x0[(size_t)g * 5 + 1], x0[(size_t)g * 5 + 2], x0[(size_t)g * 5 + 3], x0[(size_t)g * 5 + 4]};
    const double gx = goal[(size_t)g * 2], gy = goal[(size_t)g * 2 + 1];
    double ob[4] = {0.0, 0.0, 0.0, 0.0}, r;
    bool present;
    if (i < n_obst) load_obst_row(obst, (size_t)g * n_obst + i, ob);
    guess_geometry_row(q, (size_t)g * K, n_obst, i, r, present);
    const double amp = guess_amplitudes(q, K, n_obst, i, x[0], x[1], gx, gy, ob, r, present, i < K ? offsets[i] : 0.0);
    const double a = __shfl(amp, k);
    if (k == 0 && offsets_out && i < K) offsets_out[(size_t)g * K + i] = amp;
    if ((keep_first && k == 0) || i > N) return;
    const double dx = gx - x[0], dy = gy - x[1];
    const double L = sqrt(dx * dx + dy * dy);
    const double s = (double)i / (double)N;
    double xi[5];
    seed_stage(x, dx, dy, L, a, i, s, sin(kPi * s), cos(kPi * s), xi);
    double *Xi = X + ((size_t)inst * (N + 1) + i) * 5;
#pragma unroll
    for (int c = 0; c < 5; c++) Xi[c] = xi[c];
    if (i < N) { double *Ui = U + ((size_t)inst * N + i) * 2; Ui[0] = 0.0; Ui[1] = 0.0; }
}

__global__ __launch_bounds__(kGroupThreads) void select_best_kernel(int groups, int K, int N, double margin, int flags, const double *__restrict__ cost,
                                                                    const int32_t *__restrict__ status, double *X, double *U,
                                                                    int32_t *__restrict__ winner, double *__restrict__ best_cost,
                                                                    double *__restrict__ best_u0, const double *__restrict__ u0)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kGroupWaves + (threadIdx.x >> 6);
    if (g >= groups) return;
    const size_t base = (size_t)g * K;
    double c;
    const int w = select_member(K, margin, cost, status, base, lane, c);
    if (lane == 0) {
        winner[g] = w;
        if (best_cost) best_cost[g] = w >= 0 ? c : INFINITY;
    }
    if (best_u0 && lane < 2) {                                  // the solve's own u* words where given, else U[0] of the winner's row (the same value)
        double v = 0.0;
        if (w >= 0) v = u0 ? u0[(base + w) * 2 + lane] : U[(base + w) * (size_t)(2 * N) + lane];
        best_u0[(size_t)g * 2 + lane] = v;
    }
    if (!(flags & kSelectBroadcast) || w < 0 || K < 2) return;
    const int LX = 5 * (N + 1), LU = 2 * N;
    double xr[kSelectXRounds], ur[kSelectURounds];
    const double *xs = X + (base + w) * (size_t)LX, *us = U + (base + w) * (size_t)LU;
#pragma unroll
    for (int r = 0; r < kSelectXRounds; r++) { const int j = lane + 64 * r; xr[r] = j < LX ? xs[j] : 0.0; }
#pragma unroll
    for (int r = 0; r < kSelectURounds; r++) { const int j = lane + 64 * r; ur[r] = j < LU ? us[j] : 0.0; }
    for (int k = 0; k < K; k++) {
        if (k == w) continue;
        double *xd = X + (base + k) * (size_t)LX, *ud = U + (base + k) * (size_t)LU;
#pragma unroll
        for (int r = 0; r < kSelectXRounds; r++) { const int j = lane + 64 * r; if (j < LX) xd[j] = xr[r]; }
#pragma unroll
        for (int r = 0; r < kSelectURounds; r++) { const int j = lane + 64 * r; if (j < LU) ud[j] = ur[r]; }
    }
}

// GROUP CONTROL STEP (mpc_group_step_dev): everything a multi-start control step does behind its solve launch, in ONE launch, for every group g whose
// episode runs (ep_flags[g] bit 0 clear) -- in this order:
//   1. select      select_member on key / status; winner, best_key, best_u0 = the winner's row of the solve's u0, (0, 0) without a winner;
//   2. plant       x[g] <- F(x[g], best_u0) with dyn_step, in place;
//   3. obstacles   obst[g] advanced in place, obstacle j on lane j (a run-time count, 1 .. 32): obstacle_noise / obstacle_advance as obstacle_step_kernel;
//   4. bookkeeping the fused step's rule (rti_kernel.hpp, "plant, obstacles, episode bookkeeping") on the NEW state and the MOVED obstacles, with r_hit and the
//                  obstacle mask of row g K of the per-instance tables; lost / switched counters;
//   5. iterates    member 0 <- the winner's iterate shifted (shift_kernel's rule), members 1 .. K - 1 <- seed_stage for offsets[k] around the new x[g];
//                  without a winner member 0 is seeded too (offsets[0]).  No broadcast: no word is written that this launch overwrites;
//   6. inputs      the new x[g], obst[g], goal[g] into the K member rows of the replicated arrays, member_flags[g K + k] = ep_flags[g] & 1.
// One wavefront per group, a stage per lane where rows are formed (N + 1 <= 63), a member per lane in the selection (K <= 64), four groups per workgroup;
// no LDS, no atomics, no workgroup barrier (a wavefront that has nothing to do leaves).  HAZARDS: a wavefront touches the words of its own group alone, and
// it reads EVERYTHING it reads of them -- the winner's rows among them, which point 5 overwrites when the winner is member 1 .. K - 1 -- before its first
// store: the reads are issued above the wait below, which lets none of them be outstanding when the stores begin.  An idle group reads its flag and
// returns: none of its words is written.
struct GroupStepArgs {
    int groups, K, N, n_obst, flags;
    double margin, dt, randomness, vmax, tol_goal, r_hit;
    World world;
    const double *key; const int32_t *status; const double *u0, *goal, *offsets, *noise;
    double *x, *obst, *X, *U;
    int32_t *winner; double *best_key, *best_u0, *min_margin; int32_t *ep_flags, *ep_steps, *lost, *switched;
    double *member_x, *member_obst, *member_goal; int32_t *member_flags;
    const double *ip_rhit; const uint32_t *omask;               // the tables of the solve the step stands behind, or null
    GuessGeom geom;                                             // the guess family from geometry (read by group_step_kernel<true> alone)
};
constexpr int kGroupMarginAll = 1;                              // MPC_GROUP_MARGIN_ALL

// GEOM (mpc_set_guess_geometry): point 5 seeds members 1 .. K - 1 with guess_amplitudes on the new state and the moved obstacles instead of offsets[k].
// A template parameter, not a branch: group_step_kernel<false> is the kernel as it was, instruction for instruction, and the launch picks the instantiation.
// GEOM loads the r_safe row and the mask word of row g K ABOVE the wait like every other word of the group; the rule then works on registers (xn, ob).
template <bool GEOM>
__global__ __launch_bounds__(kGroupThreads) void group_step_kernel(const GroupStepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * kGroupWaves + (threadIdx.x >> 6));
    if (g >= a.groups) return;                                  // (wave-uniform, like every branch around a cross-lane step below)
    const int fl0 = a.ep_flags[g];
    if (fl0 & 1) return;
    const int K = a.K, N = a.N, no = a.n_obst;
    const size_t base = (size_t)g * K;
    // ---- 1. select; then every read of the group's words ----
    double best;
    const int w = select_member(K, a.margin, a.key, a.status, base, lane, best);
    double ub[2] = {0.0, 0.0};
    if (w >= 0) { ub[0] = a.u0[(base + w) * 2]; ub[1] = a.u0[(base + w) * 2 + 1]; }
    double xg[5];
#pragma unroll
    for (int c = 0; c < 5; c++) xg[c] = a.x[(size_t)g * 5 + c];
    const double gx = a.goal[(size_t)g * 2], gy = a.goal[(size_t)g * 2 + 1];
    const double off = lane < K ? a.offsets[lane] : 0.0;
    const double mm0 = a.min_margin[g];
    const int steps0 = a.ep_steps[g];
    const int lost0 = a.lost ? a.lost[g] : 0, sw0 = a.switched ? a.switched[g] : 0;
    // the winner's iterate as member 0 will hold it: lane i <= N takes X[w][min(i + 1, N)] (X[N] kept), lane i < N - 1 takes U[w][i + 1] (U[N - 1] = 0)
    double xs[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, us[2] = {0.0, 0.0};
    if (w >= 0 && lane <= N) {
        const double *Xw = a.X + ((base + w) * (size_t)(N + 1) + (lane < N ? lane + 1 : N)) * 5;
#pragma unroll
        for (int c = 0; c < 5; c++) xs[c] = Xw[c];
        if (lane < N - 1) { const double *Uw = a.U + ((base + w) * (size_t)N + lane + 1) * 2; us[0] = Uw[0]; us[1] = Uw[1]; }
    }
    // ---- 2. plant (every lane, the same value) ----
    double xn[5];
    dyn_step<false>(xg, ub, a.dt, xn, nullptr, nullptr);
    // ---- 3. obstacles, and the margin of the new state to where they are now ----
    double ob[4] = {0.0, 0.0, 0.0, 0.0}, margin = INFINITY;
    if (lane < no) {
        load_obst_row(a.obst, (size_t)g * no + lane, ob);
        if (a.noise) obstacle_noise(a.randomness, a.vmax, a.noise[((size_t)g * no + lane) * 2], a.noise[((size_t)g * no + lane) * 2 + 1], ob[2], ob[3]);
        obstacle_advance(a.world, a.dt, ob[0], ob[2], ob[1], ob[3]);
        const double ddx = xn[0] - ob[0], ddy = xn[1] - ob[1];
        margin = sqrt(ddx * ddx + ddy * ddy) - (a.ip_rhit ? a.ip_rhit[base * no + lane] : a.r_hit);
        // an absent obstacle moves, but is not counted (kGroupMarginAll: it is)
        if (a.omask && !(a.flags & kGroupMarginAll) && !((omask_word(a.omask, (int)base, no) >> lane) & 1u)) margin = INFINITY;
    }
    double geom_r = 0.0;
    bool geom_on = false;
    if constexpr (GEOM) guess_geometry_row(a.geom, base, no, lane, geom_r, geom_on);
    margin = -seg_max<64>(-margin, lane);
    // ---- 4. bookkeeping ----
    int fl = fl0;
    if (xn[0] < a.world.xmin || xn[0] > a.world.xmax || xn[1] < a.world.ymin || xn[1] > a.world.ymax) fl |= 2;
    const double mm = fmin(mm0, margin);
    if (mm <= 0.0) fl |= 4;
    const double ex = xn[0] - gx, ey = xn[1] - gy;
    const bool reached = sqrt(ex * ex + ey * ey) <= a.tol_goal;
    if (reached) fl |= 1;
    // ---- every load of the group's words has returned before the first store is issued ----
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        a.winner[g] = w;
        if (a.best_key) a.best_key[g] = best;
        a.min_margin[g] = mm;
        a.ep_flags[g] = fl;
        if (!reached) a.ep_steps[g] = steps0 + 1;
        if (a.lost && w < 0) a.lost[g] = lost0 + 1;
        if (a.switched && w > 0) a.switched[g] = sw0 + 1;
    }
    if (a.best_u0 && lane < 2) a.best_u0[(size_t)g * 2 + lane] = lane ? ub[1] : ub[0];
    const double xc = lane == 0 ? xn[0] : (lane == 1 ? xn[1] : (lane == 2 ? xn[2] : (lane == 3 ? xn[3] : xn[4])));      // lane c < 5: entry c of the new state
    if (lane < 5) a.x[(size_t)g * 5 + lane] = xc;
    if (lane < no) store_obst_row(a.obst, (size_t)g * no + lane, ob);
    if (a.member_flags && lane < K) a.member_flags[base + lane] = fl & 1;
    // ---- 5. the next iterates and 6. the members' inputs ----
    const double dx = gx - xn[0], dy = gy - xn[1];
    const double L = sqrt(dx * dx + dy * dy);
    const double s = (double)lane / (double)N;
    const double sn = sin(kPi * s), cs = cos(kPi * s);          // once per lane, not once per member
    double amp = off;
    if constexpr (GEOM) amp = guess_amplitudes(a.geom, K, no, lane, xn[0], xn[1], gx, gy, ob, geom_r, geom_on, off);
    for (int k = 0; k < K; k++) {
        const double ak = __shfl(amp, k);
        double xi[5], ui[2] = {0.0, 0.0};
        if (k == 0 && w >= 0) {
#pragma unroll
            for (int c = 0; c < 5; c++) xi[c] = xs[c];
            ui[0] = us[0]; ui[1] = us[1];
        } else {
            seed_stage(xn, dx, dy, L, ak, lane, s, sn, cs, xi);
        }
        if (lane <= N) {
            double *Xi = a.X + ((base + k) * (size_t)(N + 1) + lane) * 5;
#pragma unroll
            for (int c = 0; c < 5; c++) Xi[c] = xi[c];
            if (lane < N) { double *Ui = a.U + ((base + k) * (size_t)N + lane) * 2; Ui[0] = ui[0]; Ui[1] = ui[1]; }
        }
        if (a.member_x && lane < 5) a.member_x[(base + k) * 5 + lane] = xc;
        if (a.member_goal && lane < 2) a.member_goal[(base + k) * 2 + lane] = lane ? gy : gx;
        if (a.member_obst && lane < no) store_obst_row(a.member_obst, (base + k) * (size_t)no + lane, ob);
    }
}

// ROLLOUT MERIT (mpc_rollout_merit_dev): what a plan's inputs do on the plant.  Instance b rolls its U out from x0 -- X^r_0 = x0, X^r_{i+1} = F(X^r_i, U_i) with
// dyn_step's F -- and reports the NLP objective at (X^r, U) as the solve's tail forms it, the defect of a GIVEN iterate X, the least margin of X^r to the
// obstacles and the largest violation of the state boxes by X^r.  (No reference counterpart; the defect is acados' get_residuals()[1] of the iterate.)
// x0, P and goal come from row b / members (members = K: the K members of a multi-start group share one row), U, X and every per-instance table from row b.
// One wavefront per instance, stage i on lane i (N + 1 <= 63), four instances per workgroup; no LDS, no atomics.
// The plant is a chain of integrators (adjoint_inputs uses the same fact for the transposed problem), so the rollout is not a serial chain of N steps but
// three levels of exclusive prefix sums over the stage lanes:
//   (v, om)_i = (v, om)_0 + sum_{k < i} dt u_k;   psi_i = psi_0 + sum_{k < i} (dt om_k + dt^2 / 2 u_al,k);   (x, y)_i = (x, y)_0 + sum_{k < i} (sx, sy)_k,
// (sx, sy)_k being dyn_step's own quadrature at lane k's (psi_k, v_k, om_k, u_k): four sincos per lane, all lanes at once.  A scan is six __shfl_up rounds in a
// fixed order (distances 1 .. 32), so a launch gives the same bits every run; against the serial chain a sum of <= 62 terms differs by its rounding alone.
// Cost, defect, margin and box violation are then per lane and end in one wavefront reduction each (sum, max, min, max); lane 0 stores.  The obstacle loop is a
// run-time loop (1 .. 32 obstacles, mpc_create2's handles included).  A non-finite input reaches every later stage of its own instance and so its merit; the
// lanes of a wavefront hold one instance, nothing of a neighbour's is read or written.
struct MeritArgs {
    const double *U, *X;                                        // [B][N][2]; [B][N + 1][5] or null (needed for the defect alone)
    double *merit, *defect, *margin, *boxviol, *Xr;             // [B] each and [B][N + 1][5]; any of them null
    int members;
};

// exclusive prefix sums of a and b over the 64 lanes, lane 0 first: inclusive Hillis-Steele rounds, then one lane up
__device__ __forceinline__ void scan2_exclusive(double &a, double &b, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ta = __shfl_up(a, d), tb = __shfl_up(b, d);
        if (lane >= d) { a += ta; b += tb; }
    }
    const double ea = __shfl_up(a, 1), eb = __shfl_up(b, 1);
    a = lane ? ea : 0.0; b = lane ? eb : 0.0;
}

__global__ __launch_bounds__(kGroupThreads) void rollout_merit_kernel(const KParams p, const MeritArgs a)
{
    const int i = threadIdx.x & 63;
    const int inst = __builtin_amdgcn_readfirstlane(blockIdx.x * kGroupWaves + (threadIdx.x >> 6));
    if (inst >= p.batch) return;                                // (wave-uniform: every cross-lane step below runs with all 64 lanes)
    const int N = p.N, no = p.n_obst, row = inst / a.members;
    const bool act = i <= N, has_u = i < N;
    const double dt = p.dt;
    double x0v[5], gl[2], ui[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 5; c++) x0v[c] = p.x0[(size_t)row * 5 + c];
    gl[0] = p.goal[(size_t)row * 2]; gl[1] = p.goal[(size_t)row * 2 + 1];
    if (has_u) { ui[0] = a.U[((size_t)inst * N + i) * 2]; ui[1] = a.U[((size_t)inst * N + i) * 2 + 1]; }
    // ---- the rollout: three levels of scans (lanes >= N add zero) ----
    double xr[5];
    xr[3] = dt * ui[0]; xr[4] = dt * ui[1];
    scan2_exclusive(xr[3], xr[4], i);
    xr[3] += x0v[3]; xr[4] += x0v[4];
    double dpsi = has_u ? dt * xr[4] + p.h2 * ui[1] : 0.0, unused = 0.0;
    scan2_exclusive(dpsi, unused, i);
    xr[2] = x0v[2] + dpsi;
    double sx = 0.0, sy = 0.0;
    if (has_u) {
        const double xs[5] = {0.0, 0.0, xr[2], xr[3], xr[4]};
        double xn[5];
        dyn_step<false>(xs, ui, dt, xn, nullptr, nullptr);
        sx = xn[0]; sy = xn[1];
    }
    scan2_exclusive(sx, sy, i);
    xr[0] = x0v[0] + sx; xr[1] = x0v[1] + sy;
    if (a.Xr && act) {
#pragma unroll
        for (int c = 0; c < 5; c++) a.Xr[((size_t)inst * (N + 1) + i) * 5 + c] = xr[c];
    }
    // ---- the NLP objective at (X^r, U) with everything the solve's tail uses for this instance, and the margin ----
    if (a.merit || a.margin) {
        const double ex = x0v[0] - gl[0], ey = x0v[1] - gl[1];                                  // slack schedule, robot_ocp_problem.py:145-152
        const double scale = p.slack_a * (ex * ex + ey * ey + x0v[3] * x0v[3] + x0v[4] * x0v[4] + p.slack_b);
        const double alpha_i = p.alpha ? p.alpha[(size_t)inst * (N + 1) + (act ? i : N)] : scale * (double)(N - i) / (double)N;
        const double zpen = alpha_i * (has_u ? p.ss : 1.0);
        double J = 0.0, margin = INFINITY;
        if (act) {
            double r[6];
            load_ref_or_goal<true>(p.yref, p.ref_off, p.ref_T, inst, i, has_u, gl, r);
            if (p.ip_w) {
                IpConst *pw = ip_const(p.ip_w, (size_t)inst * kIpW);
                const double wg[6] = {pw[kIpWg], pw[kIpWg + 1], pw[kIpWg + 2], pw[kIpWg + 3], pw[kIpWg + 4], pw[kIpWg + 5]};
                const double we[4] = {pw[kIpWe], pw[kIpWe + 1], pw[kIpWe + 2], pw[kIpWe + 3]};
                J = ls_cost_ref(wg, we, xr, ui, r, has_u);
            } else {
                J = ls_cost_ref(p.Wg, p.Weg, xr, ui, r, has_u);
            }
            const uint32_t present = p.omask ? omask_word(p.omask, inst, no) : 0xffffffffu;
            const double *Pg = p.P + ((size_t)row * (N + 1) + i) * no * 2;
            for (int j = 0; j < no; j++) {
                if (!((present >> j) & 1u)) continue;           // an absent obstacle: no penalty, no margin; its words of P are not read
                const double dx = xr[0] - Pg[2 * j], dy = xr[1] - Pg[2 * j + 1], d2 = dx * dx + dy * dy;
                const double hv = d2 - (p.ip_r2 ? p.ip_r2[(size_t)inst * no + j] : p.r2);
                const double v = hv < 0 ? -hv : 0.0;
                J += zpen * (v + 0.5 * v * v);
                if (i >= 1) margin = fmin(margin, sqrt(d2) - (p.ip_rhit ? p.ip_rhit[(size_t)inst * no + j] : p.r_hit));
            }
        }
        if (a.merit) { J = seg_sum<64>(J, i); if (i == 0) a.merit[inst] = J; }
        if (a.margin) { margin = -seg_max<64>(-margin, i); if (i == 0) a.margin[inst] = margin; }
    }
    // ---- the defect of the given iterate: max(|X_0 - x0|, max_i |X_{i+1} - F(X_i, U_i)|) ----
    if (a.defect) {
        double def = 0.0;
        if (has_u) {
            const double *Xg = a.X + ((size_t)inst * (N + 1) + i) * 5;
            const double xi[5] = {Xg[0], Xg[1], Xg[2], Xg[3], Xg[4]};
            double xn[5];
            dyn_step<false>(xi, ui, dt, xn, nullptr, nullptr);
#pragma unroll
            for (int c = 0; c < 5; c++) {
                def = fmax(def, fabs(Xg[5 + c] - xn[c]));
                if (i == 0) def = fmax(def, fabs(xi[c] - x0v[c]));
            }
        }
        def = seg_max<64>(def, i);
        if (i == 0) a.defect[inst] = def;
    }
    // ---- the largest violation of the instance's state boxes by X^r: x, y, v, om at the stages that have the rows ----
    if (a.boxviol) {
        double viol = 0.0;
        if (i >= 1 && (i < N || (i == N && p.bx_terminal))) {
            const double xs[4] = {xr[0], xr[1], xr[3], xr[4]};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const double lo = p.ip_b ? p.ip_b[(size_t)inst * kIpB + kIpBxLo + c] : p.bx_lo[c];
                const double hi = p.ip_b ? p.ip_b[(size_t)inst * kIpB + kIpBxHi + c] : p.bx_hi[c];
                viol = fmax(viol, fmax(lo - xs[c], xs[c] - hi));
            }
        }
        viol = seg_max<64>(viol, i);
        if (i == 0) a.boxviol[inst] = viol;
    }
}

// EPISODE REFILL (mpc_episode_refill_dev): a sweep over more seeds than there are slots streams the seeds through the slots -- in front of every
// fused control step, a slot whose episode has ended (ep_flags bit 0: goal reached, robot_ocp_problem.py:247-250; or ep_steps >= max_steps: the budget of
// experiments.py:20-36) parks its result row under its seed index and starts the next seed that has not been started yet.  Two launches:
//   refill_decide_kernel, ONE workgroup: reads the finished state of every slot and hands the remaining seed indices to the finished slots in ascending
//     slot order -- an exclusive scan of the finished flags (wavefront ballot + population count, wave totals through LDS, a running base over chunks of
//     kRefillThreads slots).  No atomic, nothing that depends on the order workgroups run in: the seed-to-slot schedule is a function of the episode
//     lengths alone (with three instances per wavefront an episode's rounding depends on its neighbours, so a sweep is reproducible only if this is).
//     It writes assign[slot] and the cursor and NOTHING the decision reads;
//   refill_apply_kernel, one thread per slot: parks, reseeds (and draws the step's noise).  Every word it writes belongs to its own slot or its own seed.
//     (refill_apply_ext_kernel: the same body with per-seed tables, the status log and / or the ring of seeded episodes, RefillExtra below.)
// assign[slot]: kRefillKeep the episode runs on; kRefillDrain it has ended and no seed is left; k >= 0 it has ended and seed index k starts here.
constexpr int kRefillThreads = 256, kRefillKeep = -2, kRefillDrain = -1;
enum { kRefillAliasBug = 1, kRefillInterpGuess = 2, kRefillDrawNoise = 4 };

__global__ __launch_bounds__(kRefillThreads) void refill_decide_kernel(int slots, int seed_count, int max_steps, const int32_t *__restrict__ ep_flags,
                                                                       const int32_t *__restrict__ ep_steps, int32_t *__restrict__ assign,
                                                                       int32_t *__restrict__ cursor)
{
    constexpr int kWaves = kRefillThreads / 64;
    __shared__ int wave_fin[kWaves];
    __shared__ int wave_live[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int handed = cursor[0];
    int run = 0;              // finished slots in the chunks before this one (the same value in every thread)
    int live = 0;             // this thread's slots that run on or start a seed
    for (int c0 = 0; c0 < slots; c0 += kRefillThreads) {        // (slots <= max_batch: a bounded number of chunks)
        const int s = c0 + t;
        const bool fin = s < slots && ((ep_flags[s] & 1) || ep_steps[s] >= max_steps);
        const unsigned long long mask = __ballot(fin);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_fin[wave] = __popcll(mask);
        __syncthreads();
        int rank = run + before, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) { if (w < wave) rank += wave_fin[w]; total += wave_fin[w]; }
        if (s < slots) {
            const int k = handed + rank;                        // (handed <= seed_count, rank < slots: no overflow below 2^31 seeds + slots)
            const bool starts = fin && k < seed_count;
            assign[s] = fin ? (starts ? k : kRefillDrain) : kRefillKeep;
            live += (!fin || starts) ? 1 : 0;
        }
        run += total;
        __syncthreads();                                        // wave_fin is rewritten by the next chunk
    }
    // live slots of the whole array: the threads' counts summed through LDS
    __shared__ int part[kRefillThreads];
    part[t] = live;
    __syncthreads();
    if (t < kWaves) {
        int sum = 0;
        for (int f = 0; f < 64; f++) sum += part[t * 64 + f];
        wave_live[t] = sum;
    }
    __syncthreads();
    if (t == 0) {
        int sum = 0;
        for (int w = 0; w < kWaves; w++) sum += wave_live[w];
        const int next = handed + run;
        cursor[0] = next < seed_count ? next : seed_count;
        cursor[1] = sum;
    }
}

// What a sweep may add to the apply launch (mpc_set_refill_tables_dev, mpc_episode_ring_dev); all device pointers, any of them null.
//   PER-SEED TABLES: row k of a source goes to row s of its destination when seed index k starts in slot s -- the destinations are the per-slot arrays the
//     solve reads in place (mpc_set_instance_params_dev, mpc_set_obstacle_mask_dev, mpc_set_instance_bounds_dev);
//   STATUS LOG: log[s] = {n2, n4, first_bad, seen} is reset when a seed starts and counted by status_log_kernel behind every fused step; a parked slot parks
//     log[s][0..2] under its seed index in res_log;
//   RING: a cache of seeded episodes (ring_fill_kernel).  Entry k % ring_cap holds generator state and obstacle states of seed index k when its tag says so;
//     a slot that starts k copies them instead of seeding, and seeds in place otherwise.  seed_src[k] = 1 (ring) / 0 (in place).
// The rule of the refill holds: every word the apply launch writes belongs to its own slot or its own seed, and it reads nothing another of its threads writes.
struct RefillExtra {
    const double *W, *We, *r_safe, *r_hit; const uint32_t *mask; const double *bounds;
    double *slot_W, *slot_We, *slot_r_safe, *slot_r_hit; uint32_t *slot_mask; double *slot_bounds;
    int32_t *log, *res_log;
    int ring_cap; const unsigned *ring_state; const double *ring_obst; const int32_t *ring_tag; int32_t *seed_src;
};

// np.random.seed(seed), then the scenario's uniform draws in the reference's order (scenario_wide_kernel's values, which are scenario_kernel's) into o[n_obst][4]:
// behind them the generator is where noise_init_kernel leaves it
__device__ __forceinline__ void seed_scenario(unsigned *st, double *o, unsigned seed, int n_obst, int scenario, double x_lo, double x_hi, double y_lo, double y_hi,
                                              double v_max, double edge)
{
#pragma clang fp contract(off)
    st[0] = seed;
    for (int k = 1; k < 624; k++) st[k] = 1812433253u * (st[k - 1] ^ (st[k - 1] >> 30)) + (unsigned)k;
    st[624] = 624u; st[625] = 0u; st[626] = 0u; st[627] = 0u;
    NoiseGen g{st};
    auto uniform = [&](double lo, double hi) { const double u = g.next_double(); return lo + (hi - lo) * u; };
    for (int j = 0; j < n_obst; j++) o[j * 4 + 0] = scenario == kScenarioRandom ? uniform(x_lo, x_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 1] = scenario == kScenarioRandom ? uniform(y_lo, y_hi) : (scenario == kScenarioEdge ? edge : 0.0);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 2] = uniform(-v_max, v_max);
    for (int j = 0; j < n_obst; j++) o[j * 4 + 3] = uniform(-v_max, v_max);
}

template <bool TABLES, bool RING>
__device__ __forceinline__ void refill_apply_body(int slots, int n_obst, int N, int scenario, unsigned seed_first, int flags, int per_seed,
                                                  double x_lo, double x_hi, double y_lo, double y_hi, double v_max, double edge,
                                                  const int32_t *__restrict__ assign, const double *__restrict__ start, const double *__restrict__ goal_src,
                                                  double *__restrict__ x0, double *__restrict__ obst, double *__restrict__ goal,
                                                  double *__restrict__ X, double *__restrict__ U, double *__restrict__ min_margin,
                                                  int32_t *__restrict__ ep_flags, int32_t *__restrict__ ep_steps, unsigned *__restrict__ state,
                                                  double *__restrict__ noise, int32_t *__restrict__ slot_seed, double *__restrict__ res_f,
                                                  int32_t *__restrict__ res_i, const RefillExtra &ex)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    const int a = assign[s];
    unsigned *st = state + (size_t)s * kNoiseStateWords;
    if (a != kRefillKeep) {
        const int old = slot_seed[s];
        if (old >= 0) {                                         // the raw words of the result row; the table's columns are formed on the host
            double *rf = res_f + (size_t)old * 6;
            rf[0] = min_margin[s];
#pragma unroll
            for (int c = 0; c < 5; c++) rf[1 + c] = x0[(size_t)s * 5 + c];
            res_i[(size_t)old * 2] = ep_flags[s]; res_i[(size_t)old * 2 + 1] = ep_steps[s];
            if constexpr (TABLES) {
                if (ex.log) {
#pragma unroll
                    for (int c = 0; c < 3; c++) ex.res_log[(size_t)old * 3 + c] = ex.log[(size_t)s * 4 + c];
                }
            }
        }
        if (a == kRefillDrain) {                                // the sweep is exhausted: the slot idles like an episode that has reached its goal
            if (old >= 0) slot_seed[s] = -1;
            const int fl = ep_flags[s];
            if (!(fl & 1)) ep_flags[s] = fl | 1;
            return;
        }
        double *o = obst + (size_t)s * n_obst * 4;
        bool cached = false;
        if constexpr (RING) {                                   // the ring is a cache: an entry whose tag is not this index is not used
            const int e = a % ex.ring_cap;
            cached = ex.ring_tag[e] == a;
            if (cached) {
                const unsigned *rs = ex.ring_state + (size_t)e * kNoiseStateWords;
                for (int k = 0; k < kNoiseStateWords; k++) st[k] = rs[k];
                const double *ro = ex.ring_obst + (size_t)e * n_obst * 4;
                for (int k = 0; k < n_obst * 4; k++) o[k] = ro[k];
            }
            if (ex.seed_src) ex.seed_src[a] = cached ? 1 : 0;
        }
        if (!cached) seed_scenario(st, o, seed_first + (unsigned)a, n_obst, scenario, x_lo, x_hi, y_lo, y_hi, v_max, edge);
        if constexpr (TABLES) {                                 // row a of every per-seed source that is given -> row s of its per-slot destination
            if (ex.W) for (int c = 0; c < 6; c++) ex.slot_W[(size_t)s * 6 + c] = ex.W[(size_t)a * 6 + c];
            if (ex.We) for (int c = 0; c < 4; c++) ex.slot_We[(size_t)s * 4 + c] = ex.We[(size_t)a * 4 + c];
            if (ex.r_safe) for (int j = 0; j < n_obst; j++) ex.slot_r_safe[(size_t)s * n_obst + j] = ex.r_safe[(size_t)a * n_obst + j];
            if (ex.r_hit) for (int j = 0; j < n_obst; j++) ex.slot_r_hit[(size_t)s * n_obst + j] = ex.r_hit[(size_t)a * n_obst + j];
            if (ex.mask) ex.slot_mask[s] = ex.mask[a];
            if (ex.bounds) for (int c = 0; c < kIpB; c++) ex.slot_bounds[(size_t)s * kIpB + c] = ex.bounds[(size_t)a * kIpB + c];
            if (ex.log) { int32_t *lg = ex.log + (size_t)s * 4; lg[0] = 0; lg[1] = 0; lg[2] = -1; lg[3] = 0; }
        }
        const size_t row = per_seed ? (size_t)a : 0;
        double xs[5];
#pragma unroll
        for (int c = 0; c < 5; c++) xs[c] = start[row * 5 + c];
        if (flags & kRefillAliasBug) { xs[3] = 0.0; xs[4] = 0.0; }      // set_initial_guess() aliases self.x0 and zeroes v, omega (defect D2)
        const double gx = goal_src[row * 2], gy = goal_src[row * 2 + 1];
#pragma unroll
        for (int c = 0; c < 5; c++) x0[(size_t)s * 5 + c] = xs[c];
        goal[(size_t)s * 2] = gx; goal[(size_t)s * 2 + 1] = gy;
        double *Xs = X + (size_t)s * (N + 1) * 5, *Us = U + (size_t)s * N * 2;
        for (int i = 0; i <= N; i++) {                          // reset_guess_kernel's arithmetic, stage by stage
            double xg[5] = {xs[0], xs[1], xs[2], 0.0, 0.0};
            if (flags & kRefillInterpGuess) interp_guess(xs, gy, i, N, xg);
#pragma unroll
            for (int c = 0; c < 5; c++) Xs[i * 5 + c] = xg[c];
            if (i < N) { Us[i * 2] = 0.0; Us[i * 2 + 1] = 0.0; }
        }
        min_margin[s] = INFINITY; ep_flags[s] = 0; ep_steps[s] = 0;
        slot_seed[s] = a;
    }
    if (flags & kRefillDrawNoise) {                             // noise_draw_kernel for the slots that run: one control step's normals
        if (a == kRefillKeep && (ep_flags[s] & 1)) return;      // (a kept slot is never finished; the guard keeps the two kernels' conditions the same)
        NoiseGen g{st};
        double *nz = noise + (size_t)s * n_obst * 2;
        for (int j = 0; j < n_obst; j++) { nz[2 * j] = g.gauss(); nz[2 * j + 1] = g.gauss(); }
    }
}

// the plain sweep: no tables, no ring -- the launch of a handle on which neither was set
__global__ __launch_bounds__(64) void refill_apply_kernel(int slots, int n_obst, int N, int scenario, unsigned seed_first, int flags, int per_seed,
                                                          double x_lo, double x_hi, double y_lo, double y_hi, double v_max, double edge,
                                                          const int32_t *__restrict__ assign, const double *__restrict__ start, const double *__restrict__ goal_src,
                                                          double *__restrict__ x0, double *__restrict__ obst, double *__restrict__ goal,
                                                          double *__restrict__ X, double *__restrict__ U, double *__restrict__ min_margin,
                                                          int32_t *__restrict__ ep_flags, int32_t *__restrict__ ep_steps, unsigned *__restrict__ state,
                                                          double *__restrict__ noise, int32_t *__restrict__ slot_seed, double *__restrict__ res_f,
                                                          int32_t *__restrict__ res_i)
{
    refill_apply_body<false, false>(slots, n_obst, N, scenario, seed_first, flags, per_seed, x_lo, x_hi, y_lo, y_hi, v_max, edge, assign, start, goal_src, x0, obst, goal,
                                    X, U, min_margin, ep_flags, ep_steps, state, noise, slot_seed, res_f, res_i, RefillExtra{});
}

// ... with per-seed tables / the status log (TABLES) and / or a ring attached (RING)
template <bool TABLES, bool RING>
__global__ __launch_bounds__(64) void refill_apply_ext_kernel(int slots, int n_obst, int N, int scenario, unsigned seed_first, int flags, int per_seed,
                                                              double x_lo, double x_hi, double y_lo, double y_hi, double v_max, double edge,
                                                              const int32_t *__restrict__ assign, const double *__restrict__ start, const double *__restrict__ goal_src,
                                                              double *__restrict__ x0, double *__restrict__ obst, double *__restrict__ goal,
                                                              double *__restrict__ X, double *__restrict__ U, double *__restrict__ min_margin,
                                                              int32_t *__restrict__ ep_flags, int32_t *__restrict__ ep_steps, unsigned *__restrict__ state,
                                                              double *__restrict__ noise, int32_t *__restrict__ slot_seed, double *__restrict__ res_f,
                                                              int32_t *__restrict__ res_i, RefillExtra ex)
{
    refill_apply_body<TABLES, RING>(slots, n_obst, N, scenario, seed_first, flags, per_seed, x_lo, x_hi, y_lo, y_hi, v_max, edge, assign, start, goal_src, x0, obst, goal,
                                    X, U, min_margin, ep_flags, ep_steps, state, noise, slot_seed, res_f, res_i, ex);
}

// GROUP REFILL (mpc_group_refill_dev): the refill for multi-start groups.  A slot is a group of K members; refill_decide_kernel runs
// unchanged on the group words, and this kernel applies its decision with one wavefront per group, four groups per workgroup as in group_step_kernel:
//   keep   (the episode runs on)         the wavefront leaves: none of the group's or its members' words is written;
//   park   (finished, slot_seed >= 0)    res_f[seed] = min_margin, x[5]; res_i[seed] = ep_flags, ep_steps, lost, switched;
//   drain  (finished, no seed left)      slot_seed = -1, ep_flags |= 1, member_flags = 1 (the member solve idles them) and nothing else;
//   start k                              lane 0 seeds the generator and takes the scenario's draws (seed_scenario: mpc_noise_init_dev's state, the values of
//                                        mpc_generate_scenarios_dev) -- the one serial part, ~2000 dependent integer steps --; the draws go to the lanes by
//                                        broadcasts, obstacle j to lane j; x = the start row as given, the goal row, the bookkeeping of a new episode; members
//                                        0 .. K - 1 seeded with seed_stage, a stage per lane, sin and cos formed once per lane; x, obst, goal into the K member
//                                        rows, member_flags = 0.  winner, best_key and best_u0 are the group step's and are not written.
// HAZARDS: the kernel overwrites the words it parks.  As in group_step_kernel a wavefront issues every load of its group's words above the wait below and
// stores only behind it; it writes words of its own group, its own members and its own seed (seed indices are handed out once), and reads none that another
// wavefront writes.  No LDS, no atomics, no workgroup barrier.  No noise is drawn: noise_draw_kernel follows on the group rows with the group flags.
struct GroupRefillArgs {
    int groups, K, N, n_obst, scenario, per_seed;
    unsigned seed_first;
    double x_lo, x_hi, y_lo, y_hi, v_max, edge;
    const int32_t *assign; const double *start, *goal_src, *offsets;
    double *x, *obst, *goal, *X, *U, *min_margin;
    int32_t *ep_flags, *ep_steps, *lost, *switched;
    unsigned *state; int32_t *slot_seed;
    double *res_f; int32_t *res_i;
    double *member_x, *member_obst, *member_goal; int32_t *member_flags;
    GuessGeom geom;                                             // the guess family from geometry (read by group_refill_apply_kernel<true> alone)
};
constexpr int kGroupRefillMaxObst = 32;                        // MPC_MAX_OBST: the scenario's draws of one group, held by lane 0 until they are dealt out

// GEOM: as in group_step_kernel -- <false> is the kernel as it was; <true> loads the r_safe row and the mask word of row g K above the wait and seeds
// members 1 .. K - 1 of a started group with guess_amplitudes on the start row and the obstacles just drawn (member 0: offsets[0], which the rule keeps).
template <bool GEOM>
__global__ __launch_bounds__(kGroupThreads) void group_refill_apply_kernel(const GroupRefillArgs a)
{
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * kGroupWaves + (threadIdx.x >> 6));
    if (g >= a.groups) return;                                  // (wave-uniform, like every branch around a cross-lane step below)
    const int as = __builtin_amdgcn_readfirstlane(a.assign[g]);
    if (as == kRefillKeep) return;
    const int K = a.K, N = a.N, no = a.n_obst;
    const size_t base = (size_t)g * K;
    // ---- every read of the group's words, and of the rows a start needs ----
    const int old = __builtin_amdgcn_readfirstlane(a.slot_seed[g]);
    const double mm0 = a.min_margin[g];
    const int fl0 = a.ep_flags[g], steps0 = a.ep_steps[g], lost0 = a.lost[g], sw0 = a.switched[g];
    double xg[5];
#pragma unroll
    for (int c = 0; c < 5; c++) xg[c] = a.x[(size_t)g * 5 + c];
    double xs[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gx = 0.0, gy = 0.0;
    if (as >= 0) {
        const size_t row = a.per_seed ? (size_t)as : 0;
#pragma unroll
        for (int c = 0; c < 5; c++) xs[c] = a.start[row * 5 + c];
        gx = a.goal_src[row * 2]; gy = a.goal_src[row * 2 + 1];
    }
    const double off = lane < K ? a.offsets[lane] : 0.0;
    double geom_r = 0.0;
    bool geom_on = false;
    if constexpr (GEOM) guess_geometry_row(a.geom, base, no, lane, geom_r, geom_on);
    // ---- every load of the group's words has returned before the first store is issued ----
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (old >= 0) {                                             // park: the raw words of the result row; the table's columns are formed on the host
        const double xo = lane == 0 ? xg[0] : (lane == 1 ? xg[1] : (lane == 2 ? xg[2] : (lane == 3 ? xg[3] : xg[4])));
        if (lane < 5) a.res_f[(size_t)old * 6 + 1 + lane] = xo;
        if (lane == 0) {
            a.res_f[(size_t)old * 6] = mm0;
            int32_t *ri = a.res_i + (size_t)old * 4;
            ri[0] = fl0; ri[1] = steps0; ri[2] = lost0; ri[3] = sw0;
        }
    }
    if (as == kRefillDrain) {                                   // the sweep is exhausted: the group idles like one that has reached its goal
        if (lane == 0) { a.slot_seed[g] = -1; a.ep_flags[g] = fl0 | 1; }
        if (lane < K) a.member_flags[base + lane] = 1;
        return;
    }
    // ---- start seed index `as`: the generator and the scenario's draws on lane 0, then obstacle j to lane j ----
    double draws[kGroupRefillMaxObst * 4] = {};
    if (lane == 0)
        seed_scenario(a.state + (size_t)g * kNoiseStateWords, draws, a.seed_first + (unsigned)as, no, a.scenario, a.x_lo, a.x_hi, a.y_lo, a.y_hi, a.v_max, a.edge);
    double ob[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < no; j++) {
#pragma unroll
        for (int c = 0; c < 4; c++) { const double v = __shfl(draws[j * 4 + c], 0); if (lane == j) ob[c] = v; }
    }
    const double xc = lane == 0 ? xs[0] : (lane == 1 ? xs[1] : (lane == 2 ? xs[2] : (lane == 3 ? xs[3] : xs[4])));      // lane c < 5: entry c of the start row
    if (lane < 5) a.x[(size_t)g * 5 + lane] = xc;
    if (lane < 2) a.goal[(size_t)g * 2 + lane] = lane ? gy : gx;
    if (lane < no) store_obst_row(a.obst, (size_t)g * no + lane, ob);
    if (lane == 0) {
        a.min_margin[g] = INFINITY; a.ep_flags[g] = 0; a.ep_steps[g] = 0; a.lost[g] = 0; a.switched[g] = 0;
        a.slot_seed[g] = as;
    }
    if (lane < K) a.member_flags[base + lane] = 0;
    // ---- the members' iterates (seed_guesses_kernel's family, keep_first = 0) and inputs ----
    const double dx = gx - xs[0], dy = gy - xs[1];
    const double L = sqrt(dx * dx + dy * dy);
    const double s = (double)lane / (double)N;
    const double sn = sin(kPi * s), cs = cos(kPi * s);          // once per lane, not once per member
    double amp = off;
    if constexpr (GEOM) amp = guess_amplitudes(a.geom, K, no, lane, xs[0], xs[1], gx, gy, ob, geom_r, geom_on, off);
    for (int k = 0; k < K; k++) {
        const double ak = __shfl(amp, k);
        double xi[5];
        seed_stage(xs, dx, dy, L, ak, lane, s, sn, cs, xi);
        if (lane <= N) {
            double *Xi = a.X + ((base + k) * (size_t)(N + 1) + lane) * 5;
#pragma unroll
            for (int c = 0; c < 5; c++) Xi[c] = xi[c];
            if (lane < N) { double *Ui = a.U + ((base + k) * (size_t)N + lane) * 2; Ui[0] = 0.0; Ui[1] = 0.0; }
        }
        if (lane < 5) a.member_x[(base + k) * 5 + lane] = xc;
        if (lane < 2) a.member_goal[(base + k) * 2 + lane] = lane ? gy : gx;
        if (lane < no) store_obst_row(a.member_obst, (base + k) * (size_t)no + lane, ob);
    }
}

// RING FILL (mpc_episode_ring_fill_dev), one thread per ring entry e.  With handed = cursor[0] (the seed indices started so far) thread e owns the one index k in
// [handed, handed + capacity) with k % capacity == e; if that index exists and the entry does not hold it yet, the thread seeds seed_first + k there -- refill_apply's
// own sequence (seed_scenario), so the state is mpc_noise_init_dev's -- and writes the tag LAST.  An entry is overwritten only by k + capacity, which is owned only once
// k has been handed out (k < handed), i.e. copied by an earlier apply launch.  No atomics, no waiting: each thread reads the cursor and its own entry, and writes its own entry.
__global__ __launch_bounds__(64) void ring_fill_kernel(int capacity, int n_obst, int scenario, unsigned seed_first, int seed_count,
                                                       double x_lo, double x_hi, double y_lo, double y_hi, double v_max, double edge,
                                                       const int32_t *__restrict__ cursor, unsigned *__restrict__ ring_state, double *__restrict__ ring_obst,
                                                       int32_t *__restrict__ ring_tag)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= capacity) return;
    const int handed = cursor[0];
    const int r = handed % capacity;
    const long long k = (long long)handed + (e >= r ? e - r : e - r + capacity);      // (handed + capacity may pass 2^31)
    if (k >= seed_count || ring_tag[e] == (int)k) return;
    seed_scenario(ring_state + (size_t)e * kNoiseStateWords, ring_obst + (size_t)e * n_obst * 4, seed_first + (unsigned)k, n_obst, scenario,
                  x_lo, x_hi, y_lo, y_hi, v_max, edge);
    ring_tag[e] = (int)k;
}

// STATUS LOG (mpc_episode_status_log_dev), behind the fused step, one thread per slot: run_episodes' status2 / status4 / first_bad arithmetic per slot.
// now = the episode steps the slot has solved (ep_steps counts the steps that did not reach the goal, bit 0 of ep_flags the one that did); if that passed `seen`, the
// slot solved at episode step `seen` and its status word is that solve's
__global__ void status_log_kernel(int slots, const int32_t *__restrict__ status, const int32_t *__restrict__ ep_flags, const int32_t *__restrict__ ep_steps,
                                  int32_t *__restrict__ log)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    int32_t *lg = log + (size_t)s * 4;
    const int now = ep_steps[s] + (ep_flags[s] & 1), seen = lg[3];
    if (now > seen) {
        const int st = status[s];
        if (st == 2) lg[0] += 1;
        if (st == 4) lg[1] += 1;
        if (st != 0 && lg[2] < 0) lg[2] = seen;
        lg[3] = now;
    }
}

// EPISODE TRACE (mpc_episode_trace_set_dev, mpc_episode_trace_dev): what run_episodes(record=True) keeps per experiment -- simX, the obstacle trajectories, the
// predicted horizons (robot_ocp_problem.py:42-49, 234-241, 270-276) -- for the seeds of a sweep that ask for it, written on the device row by row.  A traced seed
// index k owns row r = seed_row[k] of every array below (the host hands out distinct rows); slot_state[s] = {seed index the slot is tracing, episode steps seen}.
// Two launches per control step, because the refill overwrites a finished slot before anything behind it could read its last step:
//   START, behind the refill: a slot whose seed index differs from slot_state[s].seed has just started it -- the plant and obstacle states are row 0;
//   STEP, behind the fused step (and the status log): with now = ep_steps + (ep_flags & 1), the status log's "episode steps solved", a slot with now > seen
//     solved at episode step `seen` -- the states it was left in are row `now`, and u*, status, iterations and the iterate X are row `seen`.
// One wavefront per slot, four slots per workgroup.  Every lane loads the slot's words first (the same addresses in all 64 lanes: wavefront-uniform), the lanes
// then stride over the doubles of a row (coalesced on both sides: X[s] is 5 (N + 1) contiguous doubles), and lane 0 writes len and slot_state last.  The refill's
// rules hold: no atomics, no waiting, bounded loops; every word written belongs to the slot or to the seed's own row; no thread reads a word that another
// wavefront of the same launch writes (slot_state[s] and len[r] are read and written by the slot's own wavefront only).
struct TraceArrays {
    const int32_t *seed_row; int32_t *slot_state, *len;
    double *x, *obst, *u; int32_t *status, *iters; double *pred;
    int rows, max_steps;
};
constexpr int kTraceThreads = 256, kTraceStart = 0, kTraceStep = 1;

__device__ __forceinline__ void trace_copy_row(double *__restrict__ dst, const double *__restrict__ src, int n, int lane)
{
    for (int i = lane; i < n; i += 64) dst[i] = src[i];         // (n <= 5 (N + 1) or 4 n_obst: a handful of rounds)
}

__global__ __launch_bounds__(kTraceThreads) void episode_trace_kernel(int slots, int phase, int n_obst, int N, TraceArrays t, const int32_t *__restrict__ slot_seed,
                                                                      const double *__restrict__ x0, const double *__restrict__ obst, const double *__restrict__ X,
                                                                      const double *__restrict__ u0, const int32_t *__restrict__ status,
                                                                      const int32_t *__restrict__ iters, const int32_t *__restrict__ ep_flags,
                                                                      const int32_t *__restrict__ ep_steps)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * (kTraceThreads / 64) + (threadIdx.x >> 6);
    if (s >= slots) return;
    const int k = slot_seed[s];
    if (k < 0) return;                                          // drained, or never filled
    const int now = ep_steps[s] + (ep_flags[s] & 1);
    const int cur = t.slot_state[2 * s], seen = t.slot_state[2 * s + 1];
    const int r = t.seed_row[k];
    const bool traced = r >= 0 && r < t.rows;
    const int ow = 4 * n_obst;
    const size_t T1 = (size_t)t.max_steps + 1;                  // state rows of a seed
    if (phase == kTraceStart) {
        if (k == cur) return;                                   // the slot runs on
        if (traced && now != 0) {                               // the episode has stepped already: a START call was skipped -- made visible, and nothing else written
            if (lane == 0) t.len[r] = -1;
            return;
        }
        if (traced) {
            trace_copy_row(t.x + (size_t)r * T1 * 5, x0 + (size_t)s * 5, 5, lane);
            trace_copy_row(t.obst + (size_t)r * T1 * ow, obst + (size_t)s * ow, ow, lane);
            if (lane == 0) t.len[r] = 0;
        }
        if (lane == 0) { t.slot_state[2 * s] = k; t.slot_state[2 * s + 1] = 0; }
        return;
    }
    if (k != cur || seen < 0 || now <= seen) return;            // idle, or not started through a START call
    if (traced && now <= t.max_steps) {                         // (seen < now <= max_steps: every index below is inside the seed's row)
        const int st = status[s], it = iters[s];
        trace_copy_row(t.x + ((size_t)r * T1 + now) * 5, x0 + (size_t)s * 5, 5, lane);
        trace_copy_row(t.obst + ((size_t)r * T1 + now) * ow, obst + (size_t)s * ow, ow, lane);
        trace_copy_row(t.u + ((size_t)r * t.max_steps + seen) * 2, u0 + (size_t)s * 2, 2, lane);
        if (t.pred) trace_copy_row(t.pred + ((size_t)r * t.max_steps + seen) * (N + 1) * 5, X + (size_t)s * (N + 1) * 5, (N + 1) * 5, lane);
        if (lane == 0) {
            t.status[(size_t)r * t.max_steps + seen] = st; t.iters[(size_t)r * t.max_steps + seen] = it;
            t.len[r] = now;
        }
    }
    if (lane == 0) t.slot_state[2 * s + 1] = now;
}

// GROUP RECORD (mpc_group_record_set_dev, mpc_group_record_dev): the closed-loop record of the multi-start GROUPS that ask for it -- what the episode trace keeps
// per seed, and the K candidates the group chose among at every step.  A recorded group g owns row r = group_row[g] of every array below (the host hands out
// distinct rows).  Two launches per control step, because group_step_kernel selects the winner and overwrites the evidence in one launch (member 0 <- the shifted
// winner, members 1 .. K - 1 reseeded, x and obst moved in place):
//   SOLVED, behind the member solve (and the rollout merit) and in front of the group tail: a running group at episode step t = ep_steps[g] -- the states the
//     solve started from are row t, the candidates' keys, status words, iterations, u0 and (with cand_X) solved iterates are row t of the candidate arrays;
//   STEPPED, behind the group tail: with now = ep_steps + (ep_flags & 1), a group with now > len[r] solved at step t = len[r] -- winner, best key and the
//     applied input are row t, the states it was left in are row `now`, and lane 0 writes len[r] = now last.
// One wavefront per group, four groups per workgroup (group_step_kernel's launch shape).  Every lane loads the group's words first (the same addresses in all 64
// lanes: wavefront-uniform); a group that is idle, unrecorded or past its rows leaves there.  The lanes then stride over the doubles of a row, 8 bytes per lane
// and round: the K (N + 1) 5 doubles of a group's member iterates are contiguous in X, and so is their row in cand_X, so both sides are coalesced (rows are
// not 16-byte aligned in general -- K (N + 1) 5 may be odd -- so no wider access is used).  The rules of the refill and the trace hold: no atomics, no LDS, no
// waiting, loops bounded by ceil(K (N + 1) 5 / 64); every word written belongs to the group's own row; no thread reads a word that another wavefront of the
// same launch writes (len[r] is read and written by the group's own wavefront only); every input is read-only here.
struct GroupRecordArrays {
    const int32_t *group_row; int32_t *len;
    double *x, *obst, *u; int32_t *winner; double *best_key, *cand_key; int32_t *cand_status, *cand_iters; double *cand_u0, *cand_X;
    int rows, max_steps;
};
constexpr int kGroupRecordSolved = 0, kGroupRecordStepped = 1;

__global__ __launch_bounds__(kGroupThreads) void group_record_kernel(int groups, int K, int phase, int n_obst, int N, GroupRecordArrays t,
                                                                     const double *__restrict__ x, const double *__restrict__ obst, const double *__restrict__ X,
                                                                     const double *__restrict__ key, const int32_t *__restrict__ status,
                                                                     const int32_t *__restrict__ iters, const double *__restrict__ u0,
                                                                     const int32_t *__restrict__ winner, const double *__restrict__ best_key,
                                                                     const double *__restrict__ best_u0, const int32_t *__restrict__ ep_flags,
                                                                     const int32_t *__restrict__ ep_steps)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kGroupWaves + (threadIdx.x >> 6);
    if (g >= groups) return;
    const int r = t.group_row[g];
    if (r < 0 || r >= t.rows) return;                           // not recorded
    const int fl = ep_flags[g], steps = ep_steps[g];
    const int T = t.max_steps, ow = 4 * n_obst;
    const size_t T1 = (size_t)T + 1;                            // state rows of a group
    const size_t base = (size_t)g * K;
    if (phase == kGroupRecordSolved) {
        if ((fl & 1) || steps < 0 || steps >= T) return;        // idle: not solved; or no row left
        const size_t at = (size_t)r * T + steps;                // (0 <= steps < T: every index below is inside the group's row)
        trace_copy_row(t.x + ((size_t)r * T1 + steps) * 5, x + (size_t)g * 5, 5, lane);
        trace_copy_row(t.obst + ((size_t)r * T1 + steps) * ow, obst + (size_t)g * ow, ow, lane);
        trace_copy_row(t.cand_key + at * K, key + base, K, lane);
        trace_copy_row(t.cand_u0 + at * K * 2, u0 + base * 2, 2 * K, lane);
        if (lane < K) { t.cand_status[at * K + lane] = status[base + lane]; t.cand_iters[at * K + lane] = iters[base + lane]; }
        if (t.cand_X) trace_copy_row(t.cand_X + at * K * (N + 1) * 5, X + base * (N + 1) * 5, K * (N + 1) * 5, lane);
        return;
    }
    const int now = steps + (fl & 1), seen = t.len[r];
    if (seen < 0 || now <= seen || now > T) return;             // idle on entry to the step, or no row left
    const size_t at = (size_t)r * T + seen;                     // (0 <= seen < now <= T)
    const int w = winner[g];
    const double bk = best_key[g];
    trace_copy_row(t.x + ((size_t)r * T1 + now) * 5, x + (size_t)g * 5, 5, lane);
    trace_copy_row(t.obst + ((size_t)r * T1 + now) * ow, obst + (size_t)g * ow, ow, lane);
    trace_copy_row(t.u + at * 2, best_u0 + (size_t)g * 2, 2, lane);
    if (lane == 0) {
        t.winner[at] = w; t.best_key[at] = bk;
        t.len[r] = now;
    }
}

// Plant integrator, robot_ocp_problem.py:207-212.
__global__ void plant_step_kernel(int batch, double dt, const double *__restrict__ x, const double *__restrict__ u, double *__restrict__ xn)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= batch) return;
    double xi[5], ui[2], xo[5];
#pragma unroll
    for (int c = 0; c < 5; c++) xi[c] = x[(size_t)t * 5 + c];
    ui[0] = u[(size_t)t * 2]; ui[1] = u[(size_t)t * 2 + 1];
    dyn_step<false>(xi, ui, dt, xo, nullptr, nullptr);
#pragma unroll
    for (int c = 0; c < 5; c++) xn[(size_t)t * 5 + c] = xo[c];
}

// The stationarity sweep of the polish on its own (tests only): the open-loop adjoint of a GIVEN per-stage gradient g[B][N+1][7] over the linearisation of a given
// iterate, through rti_kernel.hpp::adjoint_inputs in the lane layouts of the solve kernels -- G lanes per instance with one lane per stage (G = 16, 21, 32, 64), or LPS
// lanes per stage with one instance per wavefront (rti_split_kernel: the stage's first lane holds g, the others enter the suffix sums with zero).
// ru[B][N] = max(|ru_t[0]|, |ru_t[1]|), ru_t = g_u,t + B_t' pi_{t+1}, pi_t = g_x,t + A_t' pi_{t+1}.
template <int G, int LPS>
__global__ __launch_bounds__(64) void adjoint_check_kernel(KParams p, const double *__restrict__ Xin, const double *__restrict__ Uin, const double *__restrict__ gin,
                                                            double *__restrict__ ru)
{
    constexpr int IPW = LPS > 1 ? 1 : (G == 21 ? 3 : 64 / G);
    const int lane = threadIdx.x, N = p.N;
    const int slot = LPS > 1 ? 0 : (G == 21 ? seg21_slot(lane) : lane / G);
    const int i = LPS > 1 ? lane / LPS : lane - slot * G;
    const bool own = LPS > 1 ? (lane % LPS == 0) : true;
    const int inst = blockIdx.x * IPW + slot;
    const bool act = inst < p.batch && i <= N, has_u = inst < p.batch && i < N;
    double xi[5] = {0, 0, 0, 0, 0}, ui[2] = {0, 0}, g[7] = {0, 0, 0, 0, 0, 0, 0};
    StageLin S;
    S.a02 = S.a03 = S.a04 = S.a12 = S.a13 = S.a14 = S.b00 = S.b01 = S.b10 = S.b11 = 0.0; S.dt = p.dt; S.h2 = p.h2;
    if (act) {
#pragma unroll
        for (int c = 0; c < 5; c++) xi[c] = Xin[((size_t)inst * (N + 1) + i) * 5 + c];
#pragma unroll
        for (int c = 0; c < 7; c++) g[c] = gin[((size_t)inst * (N + 1) + i) * 7 + c];
    }
    if (has_u) {
        ui[0] = Uin[((size_t)inst * N + i) * 2]; ui[1] = Uin[((size_t)inst * N + i) * 2 + 1];
        double xn[5], ae[6], be[4];
        dyn_step<true>(xi, ui, p.dt, xn, ae, be);
        S.a02 = ae[0]; S.a03 = ae[1]; S.a04 = ae[2]; S.a12 = ae[3]; S.a13 = ae[4]; S.a14 = ae[5];
        S.b00 = be[0]; S.b01 = be[1]; S.b10 = be[2]; S.b11 = be[3];
    }
    const double r = adjoint_inputs<(LPS > 1 ? 64 : G)>(own && act, own && has_u, S, g, lane);
    if (own && has_u) ru[(size_t)inst * N + i] = r;
}

// ---- per-instance parameters (mpc_set_instance_params): the derived tables the IPAR kernels read ----
// What a null group falls back to, and the handle's scalings (mpc_api.hip::ip_from_config)
struct IpDefaults {
    double cs, lm_stage, lm_term;      // as make_params: cost scale of the stages (dt or 1), LM term of the stages and of the terminal stage
    double W[6], We[4], r_safe;        // mpc_config
    double r_hit, hit_off;             // the fused step's hit radius, and cfg.r_safe - r_hit
};

// Row b of the three tables from row b of W[B][6], We[B][4], r_safe[B][n_obst], r_hit[B][n_obst] (each may be null): the expressions of make_params,
// entry for entry (z order of the diagonals: ua, ual, x, y, psi, v, om; y order of the weights: x, y, v, om, ua, ual).
// Unfused arithmetic on both sides: the host compiler emits no fused multiply-add for `cs * W + lm` (make_params), device code contracts it -- also
// when written with __dmul_rn / __dadd_rn, which are plain operators in HIP's headers -- so contraction is switched off for this function's body
__host__ __device__ inline void derive_instance_params(const IpDefaults &d, int b, int n_obst, const double *W, const double *We, const double *r_safe,
                                                       const double *r_hit, double *tab_w, double *tab_r2, double *tab_rhit)
{
#pragma clang fp contract(off)
    double w[6], we[4];
    for (int k = 0; k < 6; k++) w[k] = W ? W[(size_t)b * 6 + k] : d.W[k];
    for (int k = 0; k < 4; k++) we[k] = We ? We[(size_t)b * 4 + k] : d.We[k];
    double *o = tab_w + (size_t)b * kIpW;
    o[kIpHs + 0] = d.cs * w[4] + d.lm_stage; o[kIpHs + 1] = d.cs * w[5] + d.lm_stage;
    o[kIpHs + 2] = d.cs * w[0] + d.lm_stage; o[kIpHs + 3] = d.cs * w[1] + d.lm_stage; o[kIpHs + 4] = d.lm_stage;
    o[kIpHs + 5] = d.cs * w[2] + d.lm_stage; o[kIpHs + 6] = d.cs * w[3] + d.lm_stage;
    o[kIpHt + 0] = we[0] + d.lm_term; o[kIpHt + 1] = we[1] + d.lm_term; o[kIpHt + 2] = d.lm_term;
    o[kIpHt + 3] = we[2] + d.lm_term; o[kIpHt + 4] = we[3] + d.lm_term;
    for (int k = 0; k < 6; k++) o[kIpWg + k] = d.cs * w[k];
    for (int k = 0; k < 4; k++) o[kIpWe + k] = we[k];
    for (int j = 0; j < n_obst; j++) {
        const size_t e = (size_t)b * n_obst + j;
        const double rs = r_safe ? r_safe[e] : d.r_safe;
        tab_r2[e] = rs * rs;
        tab_rhit[e] = r_hit ? r_hit[e] : (r_safe ? rs - d.hit_off : d.r_hit);
    }
}

__global__ void instance_params_kernel(IpDefaults d, int batch, int n_obst, const double *__restrict__ W, const double *__restrict__ We,
                                       const double *__restrict__ r_safe, const double *__restrict__ r_hit, double *__restrict__ tab_w,
                                       double *__restrict__ tab_r2, double *__restrict__ tab_rhit)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) derive_instance_params(d, b, n_obst, W, We, r_safe, r_hit, tab_w, tab_r2, tab_rhit);
}

// Dense dump of the linearisation of the iterate (tests only): same device functions the solve kernel uses.  REF: the gradient against the per-stage
// reference (KParams::yref) instead of the goal, formed as the REF solve kernels form it.  IPAR: the instance's own weights and the obstacles' own radii
// (KParams::ip_w, ip_r2), on the REF code with the goal as the reference where none is set
template <bool REF = false, bool IPAR = false>
__global__ void linearize_kernel(KParams p, int n_obst, const double *__restrict__ Xin, const double *__restrict__ Uin,
                                 double *__restrict__ A, double *__restrict__ B, double *__restrict__ b, double *__restrict__ q,
                                 double *__restrict__ hval, double *__restrict__ dh)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = p.N;
    if (t >= p.batch * (N + 1)) return;
    const int inst = t / (N + 1), i = t - inst * (N + 1);
    const double *Xg = Xin + (size_t)inst * (N + 1) * 5, *Ug = Uin + (size_t)inst * N * 2;
    double xi[5], ui[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < 5; c++) xi[c] = Xg[i * 5 + c];
    const double gx = p.goal[(size_t)inst * 2], gy = p.goal[(size_t)inst * 2 + 1];
    double *qo = q + (size_t)t * 7;
    static_assert(!IPAR || REF, "the per-instance parameters are built on the per-stage reference's code");
    // IPAR: this instance's weights from its row of the derived table, the goal as the reference where none is set
    const double *const ipw = IPAR ? p.ip_w + (size_t)inst * kIpW : nullptr;
    const double gl[2] = {gx, gy};
    if (i < N) {
        ui[0] = Ug[i * 2]; ui[1] = Ug[i * 2 + 1];
        double xn[5], ae[6], be[4];
        dyn_step<true>(xi, ui, p.dt, xn, ae, be);
        double *Ao = A + ((size_t)inst * N + i) * 25, *Bo = B + ((size_t)inst * N + i) * 10, *bo = b + ((size_t)inst * N + i) * 5;
        for (int c = 0; c < 25; c++) Ao[c] = 0.0;
        for (int c = 0; c < 10; c++) Bo[c] = 0.0;
        for (int c = 0; c < 5; c++) { Ao[c * 5 + c] = 1.0; bo[c] = xn[c] - Xg[(i + 1) * 5 + c]; }
        Ao[0 * 5 + 2] = ae[0]; Ao[0 * 5 + 3] = ae[1]; Ao[0 * 5 + 4] = ae[2];
        Ao[1 * 5 + 2] = ae[3]; Ao[1 * 5 + 3] = ae[4]; Ao[1 * 5 + 4] = ae[5];
        Ao[2 * 5 + 4] = p.dt;
        Bo[0] = be[0]; Bo[1] = be[1]; Bo[2] = be[2]; Bo[3] = be[3];
        Bo[2 * 2 + 1] = p.h2; Bo[3 * 2 + 0] = p.dt; Bo[4 * 2 + 1] = p.dt;
        if constexpr (IPAR) {
            const double *Wg = ipw + kIpWg;
            double r[6];
            load_ref_or_goal<IPAR>(p.yref, p.ref_off, p.ref_T, inst, i, true, gl, r);
            qo[0] = Wg[4] * (ui[0] - r[4]); qo[1] = Wg[5] * (ui[1] - r[5]);
            qo[2] = Wg[0] * (xi[0] - r[0]); qo[3] = Wg[1] * (xi[1] - r[1]); qo[4] = 0.0; qo[5] = Wg[2] * (xi[3] - r[2]); qo[6] = Wg[3] * (xi[4] - r[3]);
        } else if constexpr (REF) {
            double r[6];
            load_ref(p, inst, i, true, r);
            qo[0] = p.Wg[4] * (ui[0] - r[4]); qo[1] = p.Wg[5] * (ui[1] - r[5]);
            qo[2] = p.Wg[0] * (xi[0] - r[0]); qo[3] = p.Wg[1] * (xi[1] - r[1]); qo[4] = 0.0; qo[5] = p.Wg[2] * (xi[3] - r[2]); qo[6] = p.Wg[3] * (xi[4] - r[3]);
        } else {
        qo[0] = p.Wg[4] * ui[0]; qo[1] = p.Wg[5] * ui[1];
        qo[2] = p.Wg[0] * (xi[0] - gx); qo[3] = p.Wg[1] * (xi[1] - gy); qo[4] = 0.0; qo[5] = p.Wg[2] * xi[3]; qo[6] = p.Wg[3] * xi[4];
        }
    } else if constexpr (IPAR) {
        const double *Weg = ipw + kIpWe;
        double r[6];
        load_ref_or_goal<IPAR>(p.yref, p.ref_off, p.ref_T, inst, i, false, gl, r);
        qo[0] = qo[1] = 0.0;
        qo[2] = Weg[0] * (xi[0] - r[0]); qo[3] = Weg[1] * (xi[1] - r[1]); qo[4] = 0.0; qo[5] = Weg[2] * (xi[3] - r[2]); qo[6] = Weg[3] * (xi[4] - r[3]);
    } else if constexpr (REF) {
        double r[6];
        load_ref(p, inst, i, false, r);
        qo[0] = qo[1] = 0.0;
        qo[2] = p.Weg[0] * (xi[0] - r[0]); qo[3] = p.Weg[1] * (xi[1] - r[1]); qo[4] = 0.0; qo[5] = p.Weg[2] * (xi[3] - r[2]); qo[6] = p.Weg[3] * (xi[4] - r[3]);
    } else {
        qo[0] = qo[1] = 0.0;
        qo[2] = p.Weg[0] * (xi[0] - gx); qo[3] = p.Weg[1] * (xi[1] - gy); qo[4] = 0.0; qo[5] = p.Weg[2] * xi[3]; qo[6] = p.Weg[3] * xi[4];
    }
    const double *Pg = p.P + (size_t)t * n_obst * 2;
    for (int j = 0; j < n_obst; j++) {
        const double ex = xi[0] - Pg[2 * j], ey = xi[1] - Pg[2 * j + 1];
        hval[(size_t)t * n_obst + j] = ex * ex + ey * ey - (IPAR ? p.ip_r2[(size_t)inst * n_obst + j] : p.r2);
        dh[((size_t)t * n_obst + j) * 2] = 2 * ex; dh[((size_t)t * n_obst + j) * 2 + 1] = 2 * ey;
    }
}

}  // namespace mpc
