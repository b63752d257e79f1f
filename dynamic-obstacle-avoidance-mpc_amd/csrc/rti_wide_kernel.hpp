// rti_wide_kernel.hpp -- the RTI solve kernel for 11 .. 32 OBSTACLES: one instance per WORKGROUP of W wavefronts, LPS = 2 lanes per horizon
// stage in every wavefront (N <= 31).
//
// Same mathematics, same interior point method and the same row-parallel stage recursions as rti_split_kernel (rti_split_kernel.hpp); what
// changes is how many wavefronts hold the inequality rows.  A stage's obstacle rows live in the registers of the lanes that own the stage, and
// rti_split_kernel<10, 2> already holds 5 row pairs per lane; 30 obstacles in one wavefront would be 15 pairs (~360 registers of row state) and spill.
// Here the obstacles are spread over W wavefronts of one workgroup:
//     CAP = 20: W = 2 (10 obstacles per wavefront),   CAP = 32: W = 4 (8 per wavefront);
// wavefront w owns obstacles w K .. w K + K - 1 (K = CAP / W), dealt over the LPS lanes of a stage exactly as in the split kernel (obstacle
// w K + s LPS + part).  Wavefront 0 also owns the box rows, stages the blocks in LDS, runs the Riccati factorisation and the vector recursions
// (rowpar_*, rti_kernel.hpp, unchanged) and stores the iterate; wavefronts 1 .. W - 1 hold obstacle rows only and skip the sweeps (wave-uniform branch).
//
// What crosses wavefronts goes through LDS behind workgroup barriers (never inside a wave-divergent region), always combined in the fixed wave order
// 0, 1, .., W - 1, so that the result is deterministic and every wavefront takes the same interior-point decisions on the same scalars:
//   per stage:    the obstacle rows' barrier terms of the reduced Hessian and their share of the predictor's right-hand side (5 words), their share of the
//                 corrector's right-hand side (2), their share of C'lam in the stationarity residual (2) -- to wavefront 0;
//                 the (x, y) part of the affine and of the combined Newton step -- from wavefront 0 (the only part an obstacle row reads);
//   per instance: mu / complementarity sums and c_max (with wavefront 0's polish indicators (b)), the primal and dual step-length ratios, the affine
//                 complementarity, the stationarity residual, the item count and the initial residual, the finite-step test and the cost.
// Barriers per interior-point iteration: 8 (head, predictor in / out, affine ratios, affine complementarity, corrector in / out, combined ratios),
// +2 in the iterations that form the stationarity residual.
#pragma once
#include "rti_split_kernel.hpp"

namespace mpc {

template <int CAP>
struct WideShape {
    static_assert(CAP == 20 || CAP == 32, "row capacities 20 (two wavefronts) and 32 (four wavefronts)");
    static constexpr int W = CAP == 20 ? 2 : 4;     // wavefronts per instance
    static constexpr int K = CAP / W;               // obstacles per wavefront
};

// dynamic LDS of one instance, in doubles: dense stage blocks (RowLds), their results, the look-ahead positions of all CAP slots, then the exchange
// regions (XS: per wavefront and stage 5 words; ZA, ZD: (x, y) of the affine / combined step per stage; SC: per reduction site and wavefront 4 words)
// and a rear padding behind them (the vector recursions request operands of result blocks ahead of the last stage: reads only)
template <int CAP>
struct WideLds {
    static constexpr int W = WideShape<CAP>::W;
    static constexpr int kSites = 8;
    static __host__ __device__ constexpr int results(int N) { return (N + 1) * RowLds::HS; }
    static __host__ __device__ constexpr int positions(int N, bool lookahead) { return lookahead ? (N + 1) * CAP * 2 : 0; }
    static __host__ __device__ constexpr int exchange(int N) { return W * (N + 1) * 5 + 4 * (N + 1) + kSites * W * 4; }
    static __host__ __device__ constexpr int total(int N, bool lookahead)
    {
        return RowLds::total(N, 1) + results(N) + positions(N, lookahead) + exchange(N) + RowLds::pad_rear();
    }
};

// exchange sites (SC rows): one per reduction point of an iteration, so that a site's words are rewritten only after later barriers have passed
enum WideSite { kSiteInit = 0, kSiteHead = 1, kSiteAff = 2, kSiteMaff = 3, kSiteStep = 4, kSiteRes = 5, kSiteFin = 6, kSiteCost = 7 };

// workgroup barrier with workgroup-scope ordering of the LDS accesses around it
__device__ __forceinline__ void group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// MASKED: fewer obstacles than row pairs (p.n_obst < CAP): the run-time count, as in rti_split_kernel
// IPAR: per-instance cost constants and per-obstacle radii, as in rti_split_kernel (built on the REF code)
// OSEL: per-instance obstacle masks, as in rti_split_kernel (the word is the same in every wavefront of the workgroup)
// IBND: per-instance box bounds, as in rti_split_kernel (the row is the same in every wavefront of the workgroup)
// NSQP: up to KParams::sqp_max SQP iterations in one launch (mpc_set_sqp), as in rti_split_kernel; wavefront 0, which alone holds every stage's whole step,
// hands the updated iterate to the others through the XS words, and the exit is workgroup-uniform (the step norm travels with the finite-step test, kSiteFin)
template <int CAP, int LPS, bool MASKED = false, bool REF = false, bool IPAR = false, bool OSEL = false, bool IBND = false, bool NSQP = false>
__global__ __launch_bounds__(64 * WideShape<CAP>::W, 1) void rti_wide_kernel(const KParams p)
{
    static_assert(!NSQP || IBND, "the SQP loop is built on the per-instance bounds' code");
    static_assert(!OSEL || (IPAR && MASKED), "the obstacle masks are built on the per-instance parameters' code with a run-time row count");
    static_assert(!IBND || OSEL, "the per-instance bounds are built on the obstacle masks' code");
    static_assert(!IPAR || REF, "the per-instance parameters are built on the per-stage reference's code");
    static_assert(LPS == 2, "two lanes per horizon stage (N <= 31)");
    constexpr int W = WideShape<CAP>::W, KW = WideShape<CAP>::K;
    constexpr int NBL = 6 / LPS, NSL = KW / LPS;
    static_assert(NSL * LPS == KW, "a wavefront's obstacles fill its lanes' slots");
    constexpr int kKK = 45;
    const int tid = threadIdx.x;
    const int wv = (int)__builtin_amdgcn_readfirstlane((unsigned)(tid >> 6));      // this wavefront: wave-uniform by construction
    const bool w0 = (wv == 0);
    const int lane = tid & 63;
    const int inst = p.order ? p.order[blockIdx.x] : (int)blockIdx.x;
    const int N = p.N;
    const int nact = MASKED ? p.n_obst : CAP;
    const int i = lane / LPS;
    const int h = lane - i * LPS;
    const bool own = (h == 0);
    // OSEL: this instance's word (a scalar load) and the obstacle an absent slot reads in its place
    uint32_t omask = 0u;
    if constexpr (OSEL) omask = omask_word(p.omask, __builtin_amdgcn_readfirstlane(inst), nact);
    const int osub = OSEL ? 31 - __builtin_clz(omask | 1u) : 0;
#define OBST_ON(j) (OSEL ? (((omask >> (j)) & 1u) != 0u) : ((j) < nact))
#define OBST_IN(j) (OSEL ? ((((omask >> (j)) & 1u) != 0u) ? (j) : osub) : ((j) < nact ? (j) : nact - 1))
    const bool act = (i <= N);
    const bool has_u = (i < N);
    const bool xb = (i >= 1) && (i < N || (i == N && p.bx_terminal));
    const double dt = p.dt, h2 = p.h2;
    int is_part1 = (h == 1), is_part2 = (h == 2);
    asm volatile("" : "+v"(is_part1), "+v"(is_part2));
    auto part_of = [&](auto sc, double a0, double a1, double a2, double a3, double a4, double a5) {
        constexpr int s = decltype(sc)::value;
        double r = nth_of_six<s>(a0, a1, a2, a3, a4, a5);
        r = is_part1 ? nth_of_six<NBL + s>(a0, a1, a2, a3, a4, a5) : r;
        if (LPS == 3) r = is_part2 ? nth_of_six<(2 * NBL + s) % 6>(a0, a1, a2, a3, a4, a5) : r;
        return r;
    };
    auto zpart_of = [&](auto sc, double v0, double v1, double v2, double v3, double v5, double v6) {
        return part_of(sc, v0, v1, v2, v3, v5, v6);
    };
    using slot0 = std::integral_constant<int, 0>; using slot1 = std::integral_constant<int, 1>; using slot2 = std::integral_constant<int, 2>;
    auto slots_of = [&](const double (&v)[7], double (&out)[NBL]) {
        out[0] = zpart_of(slot0{}, v[0], v[1], v[2], v[3], v[5], v[6]);
        out[1] = zpart_of(slot1{}, v[0], v[1], v[2], v[3], v[5], v[6]);
        if constexpr (NBL > 2) out[2] = zpart_of(slot2{}, v[0], v[1], v[2], v[3], v[5], v[6]);
    };

    // ---- load ----
    double x0v[5], gl[2];
#pragma unroll
    for (int c = 0; c < 5; c++) x0v[c] = p.x0[(size_t)inst * 5 + c];
    gl[0] = p.goal[(size_t)inst * 2]; gl[1] = p.goal[(size_t)inst * 2 + 1];
    double *Xg = p.X + (size_t)inst * (N + 1) * 5, *Ug = p.U + (size_t)inst * N * 2;
    const int ep_word = ((p.fused & kFuseMetrics) && p.ep_flags) ? p.ep_flags[inst] : 0;
    double xi[5] = {0, 0, 0, 0, 0}, ui[2] = {0, 0}, xnext[5] = {0, 0, 0, 0, 0};
    if (act) {
#pragma unroll
        for (int c = 0; c < 5; c++) xi[c] = Xg[i * 5 + c];
    }
    if (has_u) {
        ui[0] = Ug[i * 2]; ui[1] = Ug[i * 2 + 1];
#pragma unroll
        for (int c = 0; c < 5; c++) xnext[c] = Xg[(i + 1) * 5 + c];
    }
    extern __shared__ double lds_raw[];
    const RowLds RL(lds_raw + RowLds::pad_front(N), N, lds_raw + RowLds::total(N, 1));
    double *lds_P = lds_raw + RowLds::total(N, 1) + WideLds<CAP>::results(N);
    double *XS = lds_P + WideLds<CAP>::positions(N, p.obst != nullptr);      // [W][N + 1][5]
    double *ZA = XS + W * (N + 1) * 5;                                         // [N + 1][2]
    double *ZD = ZA + 2 * (N + 1);                                             // [N + 1][2]
    double *SC = ZD + 2 * (N + 1);                                             // [site][W][4]
    double *xs_own = XS + ((size_t)wv * (N + 1) + (act ? i : 0)) * 5;         // this wavefront's words of this lane's stage
    auto sc_at = [&](int site, int w) { return SC + (site * W + w) * 4; };
    // two per-instance scalars of every wavefront (wave-uniform), combined in wave order: a summed (SUM_A) or maximised, b maximised
    auto group_reduce2 = [&](int site, bool sum_a, double &a, double &b) {
        if (lane == 0) { double *q = sc_at(site, wv); q[0] = a; q[1] = b; }
        group_sync();
        const double *q0 = sc_at(site, 0);
        double ra = q0[0], rb = q0[1];
#pragma unroll
        for (int w = 1; w < W; w++) {
            const double *q = sc_at(site, w);
            ra = sum_a ? ra + q[0] : fmax(ra, q[0]); rb = fmax(rb, q[1]);
        }
        a = wave_uniform(ra); b = wave_uniform(rb);
    };
    auto of_part = [&](double v, int q) { return q == 0 ? v : (q == 1 ? from_right(v) : from_right(from_right(v))); };
    double pxy[NSL][2];
    if (p.obst) {
        if (tid < 2 * nact) {      // thread walks coordinate tid & 1 of obstacle tid >> 1 through the horizon (2 CAP <= 64 W threads)
            const int j = tid >> 1, c = tid & 1;
            const double *o = p.obst + ((size_t)inst * nact + j) * 4;
            double q = o[c], v = (c == 0 && !p.world.bug_compat_predict) ? o[2] : o[3];      // defect D1: vx = self.vy (visualization.py:69)
            const double lo = c ? p.world.ymin : p.world.xmin, hi = c ? p.world.ymax : p.world.xmax;
            lds_P[tid] = q;
            for (int k = 1; k <= N; k++) {
                coord_advance(lo, hi, dt, q, v);
                lds_P[k * CAP * 2 + tid] = q;
            }
        }
    }
    group_sync();      // (also orders the look-ahead; taken without it too, so that every wavefront passes the same barriers)
    if (p.obst) {
#pragma unroll
        for (int s = 0; s < NSL; s++) {
            const int j = wv * KW + s * LPS + h, jj = OBST_IN(j);
            const double *src = lds_P + ((act ? i : 0) * CAP + jj) * 2;
            pxy[s][0] = src[0]; pxy[s][1] = src[1];
        }
    } else {
#pragma unroll
        for (int s = 0; s < NSL; s++) {
            const int j = wv * KW + s * LPS + h, jj = OBST_IN(j);
            const double *src = p.P + (((size_t)inst * (N + 1) + (act ? i : 0)) * nact + jj) * 2;
            pxy[s][0] = src[0]; pxy[s][1] = src[1];
        }
    }
    if constexpr (OSEL) {       // an empty word: no obstacle to stand in, the slots read as the origin
        if (omask == 0u) {
#pragma unroll
            for (int s = 0; s < NSL; s++) { pxy[s][0] = 0.0; pxy[s][1] = 0.0; }
        }
    }
    const bool ep_done = (ep_word & 1) != 0;
    // NSQP: iterations run and the interior-point iterations they took; an iteration starts here, on the iterate the registers hold
    [[maybe_unused]] int sqp_k = 0, sqp_it = 0;      // (read by the NSQP instantiations alone, like the label below)
sqp_again: ;
    double fin = gl[0] + gl[1] + ui[0] + ui[1];
#pragma unroll
    for (int c = 0; c < 5; c++) fin += x0v[c] + xi[c] + xnext[c];
#pragma unroll
    for (int s = 0; s < NSL; s++) fin += pxy[s][0] + pxy[s][1];

    // ---- slack schedule, robot_ocp_problem.py:145-152 ----
    double zpen = 0.0;
    {
        const double ex = x0v[0] - gl[0], ey = x0v[1] - gl[1];
        const double scale = p.slack_a * (ex * ex + ey * ey + x0v[3] * x0v[3] + x0v[4] * x0v[4] + p.slack_b);
        const double alpha_i = p.alpha ? p.alpha[(size_t)inst * (N + 1) + (act ? i : N)] : scale * (double)(N - i) / (double)N;
        zpen = alpha_i * (has_u ? p.ss : 1.0);
    }
    const bool vs = act && (i >= 1) && (p.soft_h ? (zpen > 0.0) : true);
    const bool soft = p.soft_h != 0;

    // ---- linearise ----
    double lin0 = 0.0;
    double d0[5] = {0, 0, 0, 0, 0};
    StageLin S;
    S.a02 = S.a03 = S.a04 = S.a12 = S.a13 = S.a14 = S.b00 = S.b01 = S.b10 = S.b11 = 0.0; S.dt = dt; S.h2 = h2;
    double bb[5] = {0, 0, 0, 0, 0};
    if (has_u) {
        double xn[5], ae[6], be[4];
        dyn_step<true>(xi, ui, dt, xn, ae, be);
        S.a02 = ae[0]; S.a03 = ae[1]; S.a04 = ae[2]; S.a12 = ae[3]; S.a13 = ae[4]; S.a14 = ae[5];
        S.b00 = be[0]; S.b01 = be[1]; S.b10 = be[2]; S.b11 = be[3];
#pragma unroll
        for (int c = 0; c < 5; c++) { bb[c] = xn[c] - xnext[c]; lin0 = fmax(lin0, fabs(bb[c])); }
    }
    if (i == 0) {
#pragma unroll
        for (int c = 0; c < 5; c++) { d0[c] = x0v[c] - xi[c]; lin0 = fmax(lin0, fabs(d0[c])); }
    }
    if (w0) {
        if (own && act) {       // H~aug_t: the structural zeros once
            double *hc = RL.H + RowLds::HS * i;
#pragma unroll
            for (int e = 0; e < 64; e++) hc[e] = 0.0;
        }
        if (own && has_u) {     // W~_t = [A b B] rows 0..4; column 5 is rewritten every iteration
            double *w = RL.W + RowLds::WS * i;
            const double Wrow[5][8] = {{1.0, 0.0, S.a02, S.a03, S.a04, 0.0, S.b00, S.b01}, {0.0, 1.0, S.a12, S.a13, S.a14, 0.0, S.b10, S.b11},
                                       {0.0, 0.0, 1.0, 0.0, dt, 0.0, 0.0, h2}, {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, dt, 0.0}, {0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, dt}};
#pragma unroll
            for (int k = 0; k < 5; k++)
#pragma unroll
                for (int c = 0; c < 8; c++) w[k * 8 + c] = Wrow[k][c];
        }
    }

    // ---- box variables (wavefront 0 only: the other wavefronts carry them as absent rows) ----
    bool bp[NBL];
    double cl0[NBL], ch0[NBL], hq[NBL], hd[NBL], gc0[NBL];
    double ll[NBL], tl[NBL], lh[NBL], th[NBL], rtl[NBL], rth[NBL], zs[NBL];
    // REF: this lane's stage reference, needed only here (gc0 carries it through the interior point); the cost at the end reads it again
    double yr[REF ? 6 : 1];
    if constexpr (IPAR) load_ref_or_goal<IPAR>(p.yref, p.ref_off, p.ref_T, inst, act ? i : N, has_u, gl, yr);
    else if constexpr (REF) load_ref(p, inst, act ? i : N, has_u, yr);
    // IPAR: this instance's row of the derived cost table, the same in every lane of the workgroup (scalar loads)
    IpConst *const ipw = IPAR ? ip_const(p.ip_w, (size_t)__builtin_amdgcn_readfirstlane(inst) * kIpW) : nullptr;
    // ... and the squared radius of the obstacle of row slot s of this wavefront (rows beyond the count replicate the last obstacle, as their positions do)
#define ROW_R2(s) (IPAR ? p.ip_r2[(size_t)inst * nact + (OSEL ? OBST_IN(wv * KW + (s) * LPS + h) : (wv * KW + (s) * LPS + h < nact ? wv * KW + (s) * LPS + h : nact - 1))] : p.r2)
    // IBND: this instance's row of the bounds table, read the same way
    IpConst *const ipb = IBND ? ip_const(p.ip_b, (size_t)__builtin_amdgcn_readfirstlane(inst) * kIpB) : nullptr;
    {
        auto slot_init = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const double val = part_of(sc, ui[0], ui[1], xi[0], xi[1], xi[3], xi[4]);
            double lo, hi;      // (IBND in a branch of its own, like IPAR below)
            if constexpr (IBND) {
                lo = part_of(sc, ipb[kIpBuLo + 0], ipb[kIpBuLo + 1], ipb[kIpBxLo + 0], ipb[kIpBxLo + 1], ipb[kIpBxLo + 2], ipb[kIpBxLo + 3]);
                hi = part_of(sc, ipb[kIpBuHi + 0], ipb[kIpBuHi + 1], ipb[kIpBxHi + 0], ipb[kIpBxHi + 1], ipb[kIpBxHi + 2], ipb[kIpBxHi + 3]);
            } else {
                lo = part_of(sc, p.bu_lo[0], p.bu_lo[1], p.bx_lo[0], p.bx_lo[1], p.bx_lo[2], p.bx_lo[3]);
                hi = part_of(sc, p.bu_hi[0], p.bu_hi[1], p.bx_hi[0], p.bx_hi[1], p.bx_hi[2], p.bx_hi[3]);
            }
            const bool is_u = part_of(sc, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0) != 0.0;
            bp[s] = w0 && act && (is_u ? has_u : xb);
            // (IPAR in branches of their own, statement for statement: wrapped in one expression with the kernel arguments, or in another order, the arguments'
            // arm compiles to differently scheduled code in the instantiations that were there before)
            if constexpr (IPAR)
                hd[s] = part_of(sc, has_u ? ipw[kIpHs + 0] : 0.0, has_u ? ipw[kIpHs + 1] : 0.0, has_u ? ipw[kIpHs + 2] : ipw[kIpHt + 0],
                                has_u ? ipw[kIpHs + 3] : ipw[kIpHt + 1], has_u ? ipw[kIpHs + 5] : ipw[kIpHt + 3], has_u ? ipw[kIpHs + 6] : ipw[kIpHt + 4]);
            else
                hd[s] = part_of(sc, has_u ? p.Hd_stage[0] : 0.0, has_u ? p.Hd_stage[1] : 0.0, has_u ? p.Hd_stage[2] : p.Hd_term[0],
                                has_u ? p.Hd_stage[3] : p.Hd_term[1], has_u ? p.Hd_stage[5] : p.Hd_term[3], has_u ? p.Hd_stage[6] : p.Hd_term[4]);
            hq[s] = (is_u && !has_u) ? 1.0 : hd[s];
            double wg;
            if constexpr (IPAR)
                wg = part_of(sc, has_u ? ipw[kIpWg + 4] : 0.0, has_u ? ipw[kIpWg + 5] : 0.0, has_u ? ipw[kIpWg + 0] : ipw[kIpWe + 0], has_u ? ipw[kIpWg + 1] : ipw[kIpWe + 1],
                             has_u ? ipw[kIpWg + 2] : ipw[kIpWe + 2], has_u ? ipw[kIpWg + 3] : ipw[kIpWe + 3]);
            else
                wg = part_of(sc, has_u ? p.Wg[4] : 0.0, has_u ? p.Wg[5] : 0.0, has_u ? p.Wg[0] : p.Weg[0], has_u ? p.Wg[1] : p.Weg[1],
                             has_u ? p.Wg[2] : p.Weg[2], has_u ? p.Wg[3] : p.Weg[3]);
            if constexpr (REF) gc0[s] = wg * (val - part_of(sc, yr[4], yr[5], yr[0], yr[1], yr[2], yr[3]));
            else gc0[s] = wg * (val - part_of(sc, 0.0, 0.0, gl[0], gl[1], 0.0, 0.0));
            cl0[s] = val - lo; ch0[s] = hi - val;
            tl[s] = fmax(cl0[s], p.thr0); th[s] = fmax(ch0[s], p.thr0);
            rtl[s] = rcp_nr(tl[s]); rth[s] = rcp_nr(th[s]);
            ll[s] = p.mu0 * rtl[s]; lh[s] = p.mu0 * rth[s];
            zs[s] = 0.0;
            if (bp[s]) lin0 = fmax(lin0, fmax(tl[s] - cl0[s], th[s] - ch0[s]));
        };
        slot_init(std::integral_constant<int, 0>{});
        slot_init(std::integral_constant<int, 1>{});
        if constexpr (NBL > 2) slot_init(std::integral_constant<int, 2>{});
    }
    double hd_psi_;
    if constexpr (IPAR) hd_psi_ = has_u ? ipw[kIpHs + 4] : ipw[kIpHt + 2];
    else hd_psi_ = has_u ? p.Hd_stage[4] : p.Hd_term[2];
    const double hd_psi = hd_psi_;
    // ---- this lane's obstacle rows (slot s <-> obstacle j = wv K + s LPS + part) ----
    bool sp[NSL];
    double hh[NSL], ax[NSL], ay[NSL], sv[NSL], l1[NSL], t1[NSL], l2[NSL], t2[NSL], rt1[NSL], rt2[NSL];
#pragma unroll
    for (int s = 0; s < NSL; s++) {
        if constexpr (OSEL) sp[s] = vs && OBST_ON(wv * KW + s * LPS + h);
        else sp[s] = vs && (wv * KW + s * LPS + h < nact);
        const double ex = xi[0] - pxy[s][0], ey = xi[1] - pxy[s][1];
        hh[s] = ex * ex + ey * ey - ROW_R2(s); ax[s] = 2 * ex; ay[s] = 2 * ey;
        if (soft) {
            sv[s] = (hh[s] < 0 ? -hh[s] : 0.0) + p.thr0;
            t1[s] = fmax(hh[s] + sv[s], p.thr0);
            t2[s] = fmax(sv[s], p.thr0);
        } else {
            sv[s] = 0.0; t1[s] = fmax(hh[s], p.thr0); t2[s] = 1.0;
            if (sp[s]) lin0 = fmax(lin0, t1[s] - hh[s]);
        }
        rt1[s] = rcp_nr(t1[s]); rt2[s] = rcp_nr(t2[s]);
        l1[s] = p.mu0 * rt1[s]; l2[s] = soft ? p.mu0 * rt2[s] : 0.0;
    }
    int n_items_lane = 0;
#pragma unroll
    for (int s = 0; s < NBL; s++) n_items_lane += bp[s] ? 2 : 0;
#pragma unroll
    for (int s = 0; s < NSL; s++) n_items_lane += sp[s] ? (soft ? 2 : 1) : 0;
    double n_items = seg_sum<64>((double)n_items_lane, lane);
    if (!(fabs(fin) <= 1e300)) lin0 = INFINITY;
    lin0 = seg_max<64>(lin0, lane);
    group_reduce2(kSiteInit, true, n_items, lin0);
    const double inv_items = wave_uniform(n_items > 0 ? 1.0 / n_items : 0.0);

    double z[7] = {0, 0, 0, 0, 0, 0, 0};
    double rhoPi = 1.0;
    int it = 0;
    IpmState ipm;
    ipm.running = !ep_done;
    int &status = ipm.status, &it_done = ipm.it_done;
    bool &running = ipm.running;
    float stepl = 0.0f;
    if (!(lin0 <= 1e300)) { status = 4; running = false; }

    // polish indicator (c): the stationarity residual.  Every wavefront sums its obstacle rows' share of C'lam per stage into the stage's first lane;
    // wavefront 0 adds the others' in wave order and runs the adjoint sweep; the max-norm over the instance comes back to every wavefront.
    auto stationarity = [&]() {
        double gsh[NBL], gk[6] = {0, 0, 0, 0, 0, 0}, sx = 0.0, sy = 0.0, rsm = 0.0;
#pragma unroll
        for (int s = 0; s < NBL; s++) { gsh[s] = gc0[s] + hd[s] * zs[s] + (bp[s] ? lh[s] - ll[s] : 0.0); gk[s] = gsh[s]; }
#pragma unroll
        for (int s = 0; s < NSL; s++) if (sp[s]) {
            sx -= l1[s] * ax[s]; sy -= l1[s] * ay[s];
            if (soft) rsm = fmax(rsm, fabs(zpen * sv[s] + zpen - l1[s] - l2[s]));
        }
        double shx = sx, shy = sy;
#pragma unroll
        for (int q = 1; q < LPS; q++) {
#pragma unroll
            for (int s = 0; s < NBL; s++) gsh[s] = from_right(gsh[s]);
            shx = from_right(shx); shy = from_right(shy);
#pragma unroll
            for (int s = 0; s < NBL; s++) gk[q * NBL + s] = gsh[s];
            sx += shx; sy += shy;
        }
        if (!w0 && own && act) { xs_own[0] = sx; xs_own[1] = sy; }
        double rw = seg_max<64>(rsm, lane);
        if (lane == 0) { double *q = sc_at(kSiteRes, wv); q[1] = rw; }
        group_sync();
        if (w0) {
            if (own && act) {
#pragma unroll
                for (int w = 1; w < W; w++) { const double *o = XS + ((size_t)w * (N + 1) + i) * 5; sx += o[0]; sy += o[1]; }
            }
            const double g[7] = {gk[0], gk[1], gk[2] + sx, gk[3] + sy, hd_psi * z[4], gk[4], gk[5]};
            const double ru = adjoint_inputs<64>(own && act, own && has_u, S, g, lane);
            rw = seg_max<64>(fmax(ru, rsm), lane);
#pragma unroll
            for (int w = 1; w < W; w++) rw = fmax(rw, sc_at(kSiteRes, w)[1]);
            if (lane == 0) sc_at(kSiteRes, 0)[0] = rw;
        }
        group_sync();
        return wave_uniform(sc_at(kSiteRes, 0)[0]);
    };
    for (it = 0;; it++) {
        // ---- complementarity measures ----
        double msum = 0.0, cmax = 0.0;
#pragma unroll
        for (int s = 0; s < NBL; s++) if (bp[s]) {
            const double a = ll[s] * tl[s], b = lh[s] * th[s];
            msum += a + b;
            if (!(tl[s] <= 2 * p.tl_min || ll[s] <= 2 * p.tl_min)) cmax = fmax(cmax, a);
            if (!(th[s] <= 2 * p.tl_min || lh[s] <= 2 * p.tl_min)) cmax = fmax(cmax, b);
        }
#pragma unroll
        for (int s = 0; s < NSL; s++) if (sp[s]) {
            const double a = l1[s] * t1[s];
            msum += a;
            if (!(t1[s] <= 2 * p.tl_min || l1[s] <= 2 * p.tl_min)) cmax = fmax(cmax, a);
            if (soft) {
                const double b = l2[s] * t2[s];
                msum += b;
                if (!(t2[s] <= 2 * p.tl_min || l2[s] <= 2 * p.tl_min)) cmax = fmax(cmax, b);
            }
        }
        seg_reduce2<64, true>(msum, cmax, lane);
        // wavefront 0 alone has every stage's step: its polish indicators (b) travel with its sums and hold for every wavefront
        if (w0 && lane == 0) { double *q = sc_at(kSiteHead, 0); q[2] = ipm.want_step ? 1.0 : 0.0; q[3] = (ipm.unsolved ? 1.0 : 0.0) + (ipm.long_step ? 2.0 : 0.0); }
        group_reduce2(kSiteHead, true, msum, cmax);
        {
            const double *q = sc_at(kSiteHead, 0);
            const int fl = (int)wave_uniform(q[3]);
            ipm.want_step = wave_uniform(q[2]) != 0.0; ipm.unsolved = (fl & 1) != 0; ipm.long_step = (fl & 2) != 0;
        }
        const double mu = msum * inv_items;
        const double lin = rhoPi * lin0;
        ipm_head(p, ipm, it, mu, lin, cmax);
        if (__ballot(ipm.ask_g) != 0ull) ipm_head_g(p, ipm, it, stationarity());      // (the same decision in every wavefront)
        if (!running) break;
        ipm.cprev = wave_uniform(cmax);

        // ---- predictor (sigma = 0) ----
        double rdl[NBL], rdh[NBL];
        struct SoftT { double w1, w2, rD, be1, be2, rs, rd1, rd2; } so[NSL];
        double hdiag_[NBL], g_[NBL], ssum[5];
        {
#pragma unroll
            for (int s = 0; s < NBL; s++) {
                rdl[s] = (cl0[s] + zs[s]) - tl[s];
                rdh[s] = (ch0[s] - zs[s]) - th[s];
                double hdiag = hq[s], g = gc0[s] + hd[s] * zs[s];
                if (bp[s]) {
                    const double wl = ll[s] * rtl[s], wh = lh[s] * rth[s];
                    const double bl = (ll[s] * tl[s] + ll[s] * rdl[s]) * rtl[s], bh = (lh[s] * th[s] + lh[s] * rdh[s]) * rth[s];
                    hdiag += wl + wh;
                    g += lh[s] - ll[s];
                    g += bl - bh;
                }
                hdiag_[s] = hdiag; g_[s] = g;
            }
            double sxx = 0.0, syy = 0.0, sxy = 0.0, glx = 0.0, gly = 0.0, cbx = 0.0, cby = 0.0;
#pragma unroll
            for (int s = 0; s < NSL; s++) {
                SoftT &o = so[s];
                const double y = ax[s] * z[2] + ay[s] * z[3];
                o.w1 = l1[s] * rt1[s];
                if (soft) {
                    o.rd1 = (hh[s] + y + sv[s]) - t1[s]; o.rd2 = sv[s] - t2[s];
                    o.be1 = (l1[s] * t1[s] + l1[s] * o.rd1) * rt1[s];
                    o.w2 = l2[s] * rt2[s];
                    o.be2 = (l2[s] * t2[s] + l2[s] * o.rd2) * rt2[s];
                    o.rs = zpen * sv[s] + zpen - l1[s] - l2[s];
                    o.rD = rcp_nr(zpen + o.w1 + o.w2);
                } else {
                    o.rd1 = (hh[s] + y) - t1[s]; o.rd2 = 0.0;
                    o.be1 = (l1[s] * t1[s] + l1[s] * o.rd1) * rt1[s];
                    o.w2 = 0.0; o.be2 = 0.0; o.rs = 0.0; o.rD = 0.0;
                }
                if (sp[s]) {
                    double weff, geff;
                    if (soft) {
                        weff = o.w1 * (zpen + o.w2) * o.rD;
                        geff = (o.be1 * (zpen + o.w2) - o.w1 * (o.rs + o.be2)) * o.rD;
                    } else { weff = o.w1; geff = o.be1; }
                    sxx += weff * ax[s] * ax[s]; syy += weff * ay[s] * ay[s]; sxy += weff * ax[s] * ay[s];
                    glx -= l1[s] * ax[s]; gly -= l1[s] * ay[s];
                    cbx += geff * ax[s]; cby += geff * ay[s];
                }
            }
            ssum[0] = sxx; ssum[1] = syy; ssum[2] = sxy; ssum[3] = glx + cbx; ssum[4] = gly + cby;
        }
        double bbr[5], x_init[5];
#pragma unroll
        for (int c = 0; c < 5; c++) { bbr[c] = rhoPi * bb[c]; x_init[c] = rhoPi * d0[c]; }
        double Hk[6], gk[6], Ssum[5];
        {
            double sh_h[NBL], sh_g[NBL], sh_s[5];
#pragma unroll
            for (int s = 0; s < NBL; s++) { Hk[s] = hdiag_[s]; gk[s] = g_[s]; sh_h[s] = hdiag_[s]; sh_g[s] = g_[s]; }
#pragma unroll
            for (int e = 0; e < 5; e++) { Ssum[e] = ssum[e]; sh_s[e] = ssum[e]; }
#pragma unroll
            for (int q = 1; q < LPS; q++) {
#pragma unroll
                for (int s = 0; s < NBL; s++) { sh_h[s] = from_right(sh_h[s]); sh_g[s] = from_right(sh_g[s]); }
#pragma unroll
                for (int e = 0; e < 5; e++) sh_s[e] = from_right(sh_s[e]);
#pragma unroll
                for (int s = 0; s < NBL; s++) { Hk[q * NBL + s] = sh_h[s]; gk[q * NBL + s] = sh_g[s]; }
#pragma unroll
                for (int e = 0; e < 5; e++) Ssum[e] += sh_s[e];
            }
        }
        if (!w0 && own && act) {
#pragma unroll
            for (int e = 0; e < 5; e++) xs_own[e] = Ssum[e];
        }
        group_sync();
        StageFac F;
        F.i00 = 1.0; F.l = 0.0; F.i11 = 1.0; F.k0 = 0.0; F.k1 = 0.0;
#pragma unroll
        for (int c = 0; c < 5; c++) { F.K0[c] = 0.0; F.K1[c] = 0.0; }
        double za[7] = {0, 0, 0, 0, 0, 0, 0};
        if (w0) {
            if (own && act) {   // the other wavefronts' barrier terms, in wave order; H~aug_t and the affine column of W~_t
#pragma unroll
                for (int w = 1; w < W; w++) {
                    const double *o = XS + ((size_t)w * (N + 1) + i) * 5;
#pragma unroll
                    for (int e = 0; e < 5; e++) Ssum[e] += o[e];
                }
                const double Sxx = Ssum[0], Syy = Ssum[1], Sxy = Ssum[2], Sgx = Ssum[3], Sgy = Ssum[4];
                const double hxx = Hk[2] + Sxx, hyy = Hk[3] + Syy;
                const double gxs[5] = {gk[2] + Sgx, gk[3] + Sgy, hd_psi * z[4], gk[4], gk[5]};
                const double lu0 = gk[0], lu1 = gk[1];
                double *hc = RL.H + RowLds::HS * i;
                hc[0] = hxx; hc[1] = Sxy; hc[8] = Sxy; hc[9] = hyy; hc[18] = hd_psi; hc[27] = Hk[4]; hc[36] = Hk[5]; hc[54] = Hk[0]; hc[63] = Hk[1];
#pragma unroll
                for (int c = 0; c < 5; c++) { hc[c * 8 + 5] = gxs[c]; hc[40 + c] = gxs[c]; }
                hc[46] = lu0; hc[47] = lu1; hc[53] = lu0; hc[61] = lu1;
                if (has_u) {
#pragma unroll
                    for (int k = 0; k < 5; k++) RL.W[RowLds::WS * i + k * 8 + 5] = bbr[k];
                }
            }
            wave_sync();
            // (the sweep's term order of every earlier build: rti_kernel.hpp; rows 0..4 only, except in the one instantiation that answers the shorter sweep with
            //  more scratch, 224 -> 240 bytes: <20, 2> with REF and IPAR alone keeps the six-row form -- DESIGN.md section 4)
            constexpr bool kSixRows = CAP == 20 && LPS == 2 && !MASKED && REF && IPAR && !OSEL && !IBND && !NSQP;
            rowpar_factor<RowLds, kSweepTermsParent, kSixRows>(lane, N, RL, lane < 16, dt);
            wave_sync();
            if (has_u) {
                const double *ko = RL.R + RowLds::HS * i;
#pragma unroll
                for (int c = 0; c < 5; c++) { F.K0[c] = ko[c]; F.K1[c] = ko[8 + c]; }
                F.k0 = ko[5]; F.k1 = ko[13]; F.i00 = ko[6]; F.l = ko[7]; F.i11 = ko[14];
            }
            if (own && has_u) {
                double *acl = RL.R + RowLds::HS * i + RowVec::ACL;
                const double Ar[2][5] = {{1.0, 0.0, S.a02, S.a03, S.a04}, {0.0, 1.0, S.a12, S.a13, S.a14}};
                const double Br[2][2] = {{S.b00, S.b01}, {S.b10, S.b11}};
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    acl[0 * RowVec::RS + c] = Ar[0][c] + Br[0][0] * F.K0[c] + Br[0][1] * F.K1[c];
                    acl[1 * RowVec::RS + c] = Ar[1][c] + Br[1][0] * F.K0[c] + Br[1][1] * F.K1[c];
                    acl[2 * RowVec::RS + c] = (c == 2 ? 1.0 : (c == 4 ? dt : 0.0)) + h2 * F.K1[c];
                    acl[3 * RowVec::RS + c] = (c == 3 ? 1.0 : 0.0) + dt * F.K0[c];
                    acl[4 * RowVec::RS + c] = (c == 4 ? 1.0 : 0.0) + dt * F.K1[c];
                }
                double *cc = acl + 5;
                cc[0 * RowVec::RS] = bbr[0] + S.b00 * F.k0 + S.b01 * F.k1; cc[1 * RowVec::RS] = bbr[1] + S.b10 * F.k0 + S.b11 * F.k1;
                cc[2 * RowVec::RS] = bbr[2] + h2 * F.k1; cc[3 * RowVec::RS] = bbr[3] + dt * F.k0; cc[4 * RowVec::RS] = bbr[4] + dt * F.k1;
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 5; c++) RL.R[RowVec::X + c] = x_init[c];
            }
            wave_sync();
            rowpar_vector_fast<true>(lane, N, RL, lane < 16);
            wave_sync();
            if (act) {
                const double *xx = RL.R + RowLds::HS * i + RowVec::X;
                double u0 = F.k0, u1 = F.k1;
#pragma unroll
                for (int c = 0; c < 5; c++) { za[2 + c] = xx[c]; u0 += F.K0[c] * xx[c]; u1 += F.K1[c] * xx[c]; }
                za[0] = u0; za[1] = u1;
            }
            if (own && act) { ZA[2 * i] = za[2]; ZA[2 * i + 1] = za[3]; }
        }
        group_sync();
        if (!w0 && act) { za[2] = ZA[2 * i]; za[3] = ZA[2 * i + 1]; }

        // ---- affine step ----
        double ppl[NBL], pph[NBL], pp1[NSL], pp2[NSL];
        double smu;
        {
            double rmax = 0.0, rmaxd = 0.0;
            double dtl_[NBL], dth_[NBL], dll_[NBL], dlh_[NBL], zas[NBL];
            slots_of(za, zas);
#pragma unroll
            for (int s = 0; s < NBL; s++) {
                const double dzk = zas[s];
                dtl_[s] = dzk + rdl[s]; dth_[s] = -dzk + rdh[s];
                dll_[s] = -(ll[s] * tl[s] + ll[s] * dtl_[s]) * rtl[s]; dlh_[s] = -(lh[s] * th[s] + lh[s] * dth_[s]) * rth[s];
                ppl[s] = dll_[s] * dtl_[s]; pph[s] = dlh_[s] * dth_[s];
                if (bp[s]) {
                    rmax = fmax(rmax, fmax(-dtl_[s] * rtl[s], -dth_[s] * rth[s]));
                    rmaxd = fmax(rmaxd, fmax(fma(dtl_[s], rtl[s], 1.0), fma(dth_[s], rth[s], 1.0)));
                }
            }
            double dt1_[NSL], dl1_[NSL], dt2_[NSL], dl2_[NSL];
#pragma unroll
            for (int s = 0; s < NSL; s++) {
                const SoftT &o = so[s];
                const double y = ax[s] * za[2] + ay[s] * za[3];
                dt2_[s] = dl2_[s] = 0.0; pp2[s] = 0.0;
                if (soft) {
                    const double rsum = o.rs + o.be1 + o.be2;
                    const double ds = -(rsum + o.w1 * y) * o.rD;
                    dt1_[s] = o.rd1 + (y * (zpen + o.w2) - rsum) * o.rD;
                    dt2_[s] = o.rd2 + ds;
                    dl2_[s] = -(l2[s] * t2[s] + l2[s] * dt2_[s]) * rt2[s];
                    pp2[s] = dl2_[s] * dt2_[s];
                    if (sp[s]) { rmax = fmax(rmax, -dt2_[s] * rt2[s]); rmaxd = fmax(rmaxd, fma(dt2_[s], rt2[s], 1.0)); }
                } else dt1_[s] = o.rd1 + y;
                dl1_[s] = -(l1[s] * t1[s] + l1[s] * dt1_[s]) * rt1[s];
                pp1[s] = dl1_[s] * dt1_[s];
                if (sp[s]) { rmax = fmax(rmax, -dt1_[s] * rt1[s]); rmaxd = fmax(rmaxd, fma(dt1_[s], rt1[s], 1.0)); }
            }
            seg_reduce2<64, false>(rmax, rmaxd, lane);
            group_reduce2(kSiteAff, false, rmax, rmaxd);
            double a_aff, a_affd;
            ipm_affine_steps(rmax, rmaxd, a_aff, a_affd);
            double maff = 0.0;
#pragma unroll
            for (int s = 0; s < NBL; s++) if (bp[s])
                maff += (ll[s] + a_affd * dll_[s]) * (tl[s] + a_aff * dtl_[s]) + (lh[s] + a_affd * dlh_[s]) * (th[s] + a_aff * dth_[s]);
#pragma unroll
            for (int s = 0; s < NSL; s++) if (sp[s]) {
                maff += (l1[s] + a_affd * dl1_[s]) * (t1[s] + a_aff * dt1_[s]);
                if (soft) maff += (l2[s] + a_affd * dl2_[s]) * (t2[s] + a_aff * dt2_[s]);
            }
            maff = seg_sum<64>(maff, lane);
            double unused = 0.0;
            group_reduce2(kSiteMaff, true, maff, unused);
            maff *= inv_items;
            double sigma;
            smu = ipm_centring(maff, mu, cmax, sigma);
            if (p.trace && w0 && lane == 0) {
                double *tr = p.trace + ((size_t)inst * p.iter_max + it) * 4;
                tr[0] = mu; tr[1] = sigma; tr[3] = cmax;
            }
        }

        // ---- corrector ----
        double gc[7];
        {
            double gcs[NBL];
#pragma unroll
            for (int s = 0; s < NBL; s++) {
                const double dbl = (ppl[s] - smu) * rtl[s], dbh = (pph[s] - smu) * rth[s];
                gcs[s] = bp[s] ? dbl - dbh : 0.0;
            }
            double sgx = 0.0, sgy = 0.0;
#pragma unroll
            for (int s = 0; s < NSL; s++) if (sp[s]) {
                const double db1 = (pp1[s] - smu) * rt1[s];
                double geff;
                if (soft) {
                    const SoftT &o = so[s];
                    const double db2 = (pp2[s] - smu) * rt2[s];
                    geff = (db1 * (zpen + o.w2) - o.w1 * db2) * o.rD;
                } else geff = db1;
                sgx += geff * ax[s]; sgy += geff * ay[s];
            }
            const int zidx[6] = {0, 1, 2, 3, 5, 6};
            gc[4] = 0.0;
            double Sgx = 0.0, Sgy = 0.0;
#pragma unroll
            for (int q = 0; q < LPS; q++) {
#pragma unroll
                for (int s = 0; s < NBL; s++) gc[zidx[q * NBL + s]] = of_part(gcs[s], q);
                const double vx = of_part(sgx, q), vy = of_part(sgy, q);
                Sgx = q == 0 ? vx : Sgx + vx; Sgy = q == 0 ? vy : Sgy + vy;
            }
            if (!w0 && own && act) { xs_own[0] = Sgx; xs_own[1] = Sgy; }
            group_sync();
            if (w0) {
                if (own && act) {
#pragma unroll
                    for (int w = 1; w < W; w++) { const double *o = XS + ((size_t)w * (N + 1) + i) * 5; Sgx += o[0]; Sgy += o[1]; }
                }
                gc[2] += Sgx; gc[3] += Sgy;
                if (own && act) {
                    double *cc = RL.R + RowLds::HS * i + RowVec::CT;
#pragma unroll
                    for (int c = 0; c < 5; c++) cc[c] = gc[2 + c] + F.K0[c] * gc[0] + F.K1[c] * gc[1];
                }
                wave_sync();
                rowpar_vector_fast<false>(lane, N, RL, lane < 16);
                wave_sync();
                if (has_u) {
                    const double *pp = RL.R + RowLds::HS * (i + 1) + RowVec::P;
                    const double pv[5] = {pp[0], pp[1], pp[2], pp[3], pp[4]};
                    const double m0 = gc[0] + S.dua(pv), m1 = gc[1] + S.dual(pv);
                    F.k1 = fma(F.l, m0, -m1) * F.i11;
                    F.k0 = fma(-F.l, F.k1, -(m0 * F.i00));
                }
            }
        }
        double dz[7] = {0, 0, 0, 0, 0, 0, 0};
        if (w0) {
            if (own && has_u) {
                double *cc = RL.R + RowLds::HS * i + RowVec::ACL + 5;
                cc[0 * RowVec::RS] = S.b00 * F.k0 + S.b01 * F.k1; cc[1 * RowVec::RS] = S.b10 * F.k0 + S.b11 * F.k1;
                cc[2 * RowVec::RS] = h2 * F.k1; cc[3 * RowVec::RS] = dt * F.k0; cc[4 * RowVec::RS] = dt * F.k1;
                RL.R[RowLds::HS * i + kKK] = F.k0; RL.R[RowLds::HS * i + kKK + 1] = F.k1;
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 5; c++) RL.R[RowVec::X + c] = 0.0;
            }
            wave_sync();
            rowpar_vector_fast<true>(lane, N, RL, lane < 16);
            wave_sync();
            if (act) {
                const double *xx = RL.R + RowLds::HS * i + RowVec::X;
                double u0 = has_u ? RL.R[RowLds::HS * i + kKK] : 0.0, u1 = has_u ? RL.R[RowLds::HS * i + kKK + 1] : 0.0;
#pragma unroll
                for (int c = 0; c < 5; c++) { dz[2 + c] = xx[c]; u0 += F.K0[c] * xx[c]; u1 += F.K1[c] * xx[c]; }
                dz[0] = u0; dz[1] = u1;
            }
#pragma unroll
            for (int c = 0; c < 7; c++) dz[c] += za[c];
            if (own && act) { ZD[2 * i] = dz[2]; ZD[2 * i + 1] = dz[3]; }
        }
        group_sync();
        if (!w0 && act) { dz[2] = ZD[2 * i]; dz[3] = ZD[2 * i + 1]; }

        // ---- combined step ----
        {
            double rmax = 0.0, rmaxd = 0.0;
            double dzs[NBL], dtl_[NBL], dth_[NBL], dll_[NBL], dlh_[NBL];
            slots_of(dz, dzs);
#pragma unroll
            for (int s = 0; s < NBL; s++) {
                dtl_[s] = dzs[s] + rdl[s]; dth_[s] = -dzs[s] + rdh[s];
                dll_[s] = -(ll[s] * tl[s] - smu + ppl[s] + ll[s] * dtl_[s]) * rtl[s];
                dlh_[s] = -(lh[s] * th[s] - smu + pph[s] + lh[s] * dth_[s]) * rth[s];
                if (bp[s]) {
                    rmax = fmax(rmax, fmax(-dtl_[s] * rtl[s], -dth_[s] * rth[s]));
                    rmaxd = fmax(rmaxd, fmax(-dll_[s] * rcp_nr(ll[s]), -dlh_[s] * rcp_nr(lh[s])));
                }
            }
            double dt1_[NSL], dl1_[NSL], dt2_[NSL], dl2_[NSL], ds_[NSL];
#pragma unroll
            for (int s = 0; s < NSL; s++) {
                const SoftT &o = so[s];
                const double y = ax[s] * dz[2] + ay[s] * dz[3];
                dt2_[s] = dl2_[s] = ds_[s] = 0.0;
                if (soft) {
                    const double db1 = (pp1[s] - smu) * rt1[s], db2 = (pp2[s] - smu) * rt2[s];
                    const double rsum = o.rs + (o.be1 + db1) + (o.be2 + db2);
                    ds_[s] = -(rsum + o.w1 * y) * o.rD;
                    dt1_[s] = o.rd1 + (y * (zpen + o.w2) - rsum) * o.rD;
                    dt2_[s] = o.rd2 + ds_[s];
                    dl2_[s] = -(l2[s] * t2[s] - smu + pp2[s] + l2[s] * dt2_[s]) * rt2[s];
                    if (sp[s]) { rmax = fmax(rmax, -dt2_[s] * rt2[s]); rmaxd = fmax(rmaxd, -dl2_[s] * rcp_nr(l2[s])); }
                } else dt1_[s] = o.rd1 + y;
                dl1_[s] = -(l1[s] * t1[s] - smu + pp1[s] + l1[s] * dt1_[s]) * rt1[s];
                if (sp[s]) { rmax = fmax(rmax, -dt1_[s] * rt1[s]); rmaxd = fmax(rmaxd, -dl1_[s] * rcp_nr(l1[s])); }
            }
            seg_reduce2<64, false>(rmax, rmaxd, lane);
            group_reduce2(kSiteStep, false, rmax, rmaxd);
            double alpha, alphad;
            ipm_step_lengths(rmax, rmaxd, alpha, alphad);
            if (p.trace && w0 && lane == 0) p.trace[((size_t)inst * p.iter_max + it) * 4 + 2] = alpha;
            ipm_step_check(ipm, it, alpha, alphad, smu);
            ipm_polish_step<64>(p, ipm, lane, alpha, dz, stepl);      // (wavefront 0's verdict is the one that counts: kSiteHead)
            if (running) {
#pragma unroll
                for (int c = 0; c < 7; c++) z[c] += alpha * dz[c];
#pragma unroll
                for (int s = 0; s < NBL; s++) {
                    zs[s] += alpha * dzs[s];
                    if (bp[s]) {
                        tl[s] = fmax(tl[s] + alpha * dtl_[s], p.tl_min); th[s] = fmax(th[s] + alpha * dth_[s], p.tl_min);
                        ll[s] = fmax(ll[s] + alphad * dll_[s], p.tl_min); lh[s] = fmax(lh[s] + alphad * dlh_[s], p.tl_min);
                        rtl[s] = rcp_nr(tl[s]); rth[s] = rcp_nr(th[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < NSL; s++) if (sp[s]) {
                    t1[s] = fmax(t1[s] + alpha * dt1_[s], p.tl_min); l1[s] = fmax(l1[s] + alphad * dl1_[s], p.tl_min);
                    rt1[s] = rcp_nr(t1[s]);
                    if (soft) {
                        sv[s] += alpha * ds_[s];
                        t2[s] = fmax(t2[s] + alpha * dt2_[s], p.tl_min); l2[s] = fmax(l2[s] + alphad * dl2_[s], p.tl_min);
                        rt2[s] = rcp_nr(t2[s]);
                    }
                }
                rhoPi = wave_uniform(rhoPi * (1.0 - alpha));
            }
        }
        if (!running) break;
    }

    {
        const double *xg = p.x0 + (size_t)inst * 5, *gg = p.goal + (size_t)inst * 2;
        asm volatile("" : "+v"(xg), "+v"(gg));
#pragma unroll
        for (int c = 0; c < 5; c++) x0v[c] = xg[c];
        gl[0] = gg[0]; gl[1] = gg[1];
    }
    // ---- full step on the iterate; status 4 leaves it unchanged.  Wavefront 0 holds every stage's whole step, the others the (x, y) part.  The solve tail,
    //      shared pieces tail_* (rti_kernel.hpp) ----
    const bool store = !ep_done;
    [[maybe_unused]] double sqp_nrm = 0.0;      // NSQP: wavefront 0's step norm, the same in every wavefront behind the reduction below
    {
        double s4 = ipm_finite_step<64>(status, z, lane) == 4 ? 1.0 : 0.0, unused = 0.0;
        if constexpr (NSQP) unused = seg_max<64>(w0 ? sqp_step_norm(act, has_u, z) : 0.0, lane);      // (NSQP: the second word carries wavefront 0's step norm)
        group_reduce2(kSiteFin, false, s4, unused);
        if (s4 != 0.0) status = 4;
        if constexpr (NSQP) sqp_nrm = unused;
    }
    tail_full_step(status, z, xi, ui);
    if constexpr (NSQP) {
        // either the next iteration -- wavefront 0 publishes the iterate (7 words per stage in XS, which nothing reads between the barrier above and the
        // predictor of the next iteration), every lane of every wavefront takes its stage's state and input and the successor state the defect needs; x0 and
        // the goal have just been read again -- or the tail below, once, on the last status
        sqp_k += 1; sqp_it += it_done;
        if (!ep_done && status != 4 && sqp_k < p.sqp_max && !(sqp_nrm <= p.sqp_tol)) {
            if (w0 && own && act) {
                double *q = XS + 7 * i;
#pragma unroll
                for (int c = 0; c < 5; c++) q[c] = xi[c];
                q[5] = has_u ? ui[0] : 0.0; q[6] = has_u ? ui[1] : 0.0;
            }
            group_sync();
            {
                const double *q = XS + 7 * (act ? i : 0), *qn = XS + 7 * (has_u ? i + 1 : 0);
#pragma unroll
                for (int c = 0; c < 5; c++) { const double a = q[c], b = qn[c]; xi[c] = act ? a : 0.0; xnext[c] = has_u ? b : 0.0; }
                const double u0 = q[5], u1 = q[6];
                ui[0] = has_u ? u0 : 0.0; ui[1] = has_u ? u1 : 0.0;
            }
            group_sync();
            goto sqp_again;
        }
        it_done = sqp_it;
    }
    const double u_apply[2] = {lane_value(ui[0], 0), lane_value(ui[1], 0)};   // u* = U[0] (wavefront 0)
    tail_reset_on_fail(p.fused, status, x0v, gl[1], i, N, xi, ui);
    if (w0 && store && own && (status != 4 || (p.fused & (kFuseResetOnFail | kFuseShift)))) tail_store_iterate(p.fused, i, N, act, has_u, xi, ui, Xg, Ug);
    // NLP objective at the returned iterate: LS cost (wavefront 0's stage owners) + exact penalty of every wavefront's obstacle rows, in wave order
    if (p.cost) {
        double J = 0.0;
        if (act) {
            if (IPAR && w0 && own) {
                double r[6];
                load_ref_or_goal<IPAR>(p.yref, p.ref_off, p.ref_T, inst, i, has_u, gl, r);
                const double wg[6] = {ipw[kIpWg], ipw[kIpWg + 1], ipw[kIpWg + 2], ipw[kIpWg + 3], ipw[kIpWg + 4], ipw[kIpWg + 5]};      // (read again: not carried)
                const double we[4] = {ipw[kIpWe], ipw[kIpWe + 1], ipw[kIpWe + 2], ipw[kIpWe + 3]};
                J = ls_cost_ref(wg, we, xi, ui, r, has_u);
            } else if (REF && w0 && own) {
                const double *row = ref_row(p.yref, p.ref_off, p.ref_T, inst, i);
                const double r[6] = {row[0], row[1], row[2], row[3], has_u ? row[4] : 0.0, has_u ? row[5] : 0.0};
                J = ls_cost_ref(p.Wg, p.Weg, xi, ui, r, has_u);
            } else if (w0 && own) {
                const double ex = xi[0] - gl[0], ey = xi[1] - gl[1];
                if (has_u) J = 0.5 * (p.Wg[0] * ex * ex + p.Wg[1] * ey * ey + p.Wg[2] * xi[3] * xi[3] + p.Wg[3] * xi[4] * xi[4]
                                      + p.Wg[4] * ui[0] * ui[0] + p.Wg[5] * ui[1] * ui[1]);
                else J = 0.5 * (p.Weg[0] * ex * ex + p.Weg[1] * ey * ey + p.Weg[2] * xi[3] * xi[3] + p.Weg[3] * xi[4] * xi[4]);
            }
#pragma unroll
            for (int s = 0; s < NSL; s++) if (OBST_ON(wv * KW + s * LPS + h)) {
                const double dx = xi[0] - pxy[s][0], dy = xi[1] - pxy[s][1];
                const double hv = dx * dx + dy * dy - ROW_R2(s);
                const double v = hv < 0 ? -hv : 0.0;
                J += zpen * (v + 0.5 * v * v);
            }
        }
        J = seg_sum<64>(J, lane);
        double unused = 0.0;
        group_reduce2(kSiteCost, true, J, unused);
        if (w0 && lane == 0 && store) p.cost[inst] = J;
    }
    if (!w0) return;      // (no barrier behind this point)
    // ---- plant, obstacles, episode bookkeeping (fused closed-loop step): wavefront 0, obstacle j = lane (CAP <= 64) ----
    if (p.fused & (kFusePlant | kFuseObstacles | kFuseMetrics)) {
        double xp[5] = {x0v[0], x0v[1], x0v[2], x0v[3], x0v[4]};
        if ((p.fused & kFuseAliasBug) && (p.fused & kFuseResetOnFail) && status == 4) { xp[3] = 0.0; xp[4] = 0.0; }
        double xnew[5] = {xp[0], xp[1], xp[2], xp[3], xp[4]};
        if (p.fused & kFusePlant) dyn_step<false>(xp, u_apply, dt, xnew, nullptr, nullptr);
        if ((p.fused & kFusePlant) && lane == 0 && store && p.x0_rw) {
#pragma unroll
            for (int c = 0; c < 5; c++) p.x0_rw[(size_t)inst * 5 + c] = xnew[c];
        }
        double margin = INFINITY;
        if (p.obst && lane < nact) {
            const double *o = p.obst + ((size_t)inst * nact + lane) * 4;
            double ox = o[0], oy = o[1], ovx = o[2], ovy = o[3];
            if (p.fused & kFuseObstacles) {
                if (p.noise) obstacle_noise(p.randomness, p.vmax, p.noise[((size_t)inst * nact + lane) * 2], p.noise[((size_t)inst * nact + lane) * 2 + 1], ovx, ovy);
                obstacle_advance(p.world, dt, ox, ovx, oy, ovy);
                if (store && p.obst_rw) { double *w = p.obst_rw + ((size_t)inst * nact + lane) * 4; w[0] = ox; w[1] = oy; w[2] = ovx; w[3] = ovy; }
            }
            const double ddx = xnew[0] - ox, ddy = xnew[1] - oy;
            margin = sqrt(ddx * ddx + ddy * ddy) - (IPAR ? p.ip_rhit[(size_t)inst * nact + lane] : p.r_hit);
            if constexpr (OSEL) {       // an absent obstacle moves, but is not counted (kFuseMarginAll: it is)
                if (!OBST_ON(lane) && !(p.fused & kFuseMarginAll)) margin = INFINITY;
            }
        }
        if (p.fused & kFuseMetrics) {
            margin = -seg_max<64>(-margin, lane);
            if (lane == 0 && store) {
                int fl = p.ep_flags[inst];
                if (xnew[0] < p.world.xmin || xnew[0] > p.world.xmax || xnew[1] < p.world.ymin || xnew[1] > p.world.ymax) fl |= 2;
                const double mm = fmin(p.ep_min_margin[inst], margin);
                p.ep_min_margin[inst] = mm;
                if (mm <= 0.0) fl |= 4;
                const double gx_ = xnew[0] - gl[0], gy_ = xnew[1] - gl[1];
                if (sqrt(gx_ * gx_ + gy_ * gy_) <= p.tol_goal) fl |= 1;
                else p.ep_steps[inst] += 1;
                p.ep_flags[inst] = fl;
            }
        }
    }
    if (lane == 0 && p.u0 && store) { p.u0[(size_t)inst * 2] = u_apply[0]; p.u0[(size_t)inst * 2 + 1] = u_apply[1]; }
    if (lane == 0 && store) {
        if (p.iters_acc) p.iters_acc[inst] += it_done;
        if (p.status_acc) p.status_acc[inst] += tail_status_acc_word(status);
        if (p.status) p.status[inst] = status;
        if (p.iters) p.iters[inst] = it_done;
        if constexpr (NSQP) { if (p.sqp_iters) p.sqp_iters[inst] = sqp_k; }
    }
    if constexpr (REF) {      // the reference window moves with the plant: the last access to the offset (the prologue and the cost above read it)
        if ((p.fused & kFuseAdvanceRef) && lane == 0 && store && p.ref_off) p.ref_off[inst] += 1;
    }
}
#undef ROW_R2
#undef OBST_ON
#undef OBST_IN

}  // namespace mpc
