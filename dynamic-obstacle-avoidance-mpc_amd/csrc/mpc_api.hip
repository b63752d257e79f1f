// mpc_api.hip -- C ABI of libmpcgpu.so (include/mpc_gpu.h): handle management, launches, host<->device staging.
// No CPU fallback exists: every compute entry point launches a HIP kernel or fails.
#include "../../include/mpc_gpu.h"
#include "aux_kernels.hpp"
#include "rti_kernel.hpp"
#include "rti_split_kernel.hpp"
#include "rti_wide_kernel.hpp"
#include "solve_dispatch.hpp"

#include <cmath>
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// RCCL's ABI for the five entry points of the cost exchange, declared here: they are resolved from librccl.so.1 with dlopen on first use, so the
// library has neither a link-time nor a build-time dependency on RCCL (a ROCm install without the RCCL development headers still builds the solver;
// mpc_comm_* then fails loudly at run time if the shared object is absent too).  Values as in rccl/rccl.h (= NCCL's): ncclSuccess 0, ncclFloat64 8,
// a 128-byte unique id (tests/test_abi.py compares them with the installed header when there is one).
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[MPC_COMM_ID_BYTES]; } ncclUniqueId;
typedef int ncclResult_t;
typedef int ncclDataType_t;
static constexpr ncclResult_t ncclSuccess = 0;
static constexpr ncclDataType_t ncclDouble = 8;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, const char *a = "", const char *b = "")
{
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return fail(MPC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int kMaxEvents = 2048;   // solve launches timed per profiling window; later launches are not timed

// A per-instance feature as the host sees it.  mode: 0 off, 1 host arrays (copied into a buffer of the handle's), 2 the caller's device arrays (used in
// place); batch: the instances it covers -- those of the host arrays, max_batch for device arrays (a solve of more is refused).  feature_level, the coverage
// refusals of attach_inputs and each feature's off path (one function, which its host setter and its _dev setter both call) go by this and nothing else
struct feature { int mode, batch; };
struct ip_tables { double *w, *r2, *rhit; };     // the derived tables the IPAR kernels read (KParams::ip_w, ip_r2, ip_rhit), max_batch rows each
struct owned_buf { void *p; bool pinned; };      // one allocation of the handle's (own / disown below)

}  // namespace

struct mpc_handle {
    mpc_config cfg;
    int device, max_batch;
    hipStream_t stream;
    std::vector<owned_buf> owned;     // every device / pinned buffer that belongs to the handle (own, disown); mpc_destroy releases what is recorded here
    double *dX, *dU;                  // handle-owned iterate
    double *d_x0, *d_P, *d_goal, *d_obst, *d_u0, *d_cost, *d_xa, *d_ua, *d_xb;   // staging for the host-pointer API
    int32_t *d_status, *d_iters;
    int lanes_override;
    int use_mfma;                     // matrix-core Riccati factorisation when one instance per wavefront is chosen
    int row_parallel;                 // row-parallel (64-bit DPP) Riccati factorisation instead of the one-lane systolic sweep
    int block2;                       // stage recursions on pairs of stages where the mapping has them (mpc_set_block_riccati; default off)
    int split_override;               // lanes per horizon stage: 0 automatic, 1 one lane per stage, 2 / 3 split kernel (mpc_set_lanes_per_stage)
    int waves_override;               // wavefronts per SIMD of the split kernel: 0 automatic, 1, 2 (mpc_set_waves_per_simd)
    int simd_count;                   // SIMDs of the device (4 per compute unit)
    int profiling;                    // 0 off, k > 0: HIP events around every k-th solve launch
    int launch_count;
    double *d_trace;                  // optional debug trace buffer (mpc_debug_trace)
    int32_t *d_iters_acc, *d_status_acc;   // optional accumulators (mpc_set_accumulators)
    int scheduling;                   // instance scheduling for the mappings that pack several instances into a wavefront (mpc_set_instance_scheduling)
    int32_t *d_order, *d_iters_sched; // ... the order for the next launch, and the iteration counts it is built from when the caller asks for none
    unsigned *d_sched_hist;           // ... per-block histograms of the counting sort [bins][blocks]
    int order_batch;                  // batch size d_order is a permutation of (0 = none yet)
    feature alpha;                    // explicit slack schedule (mpc_set_slack_schedule[_dev])
    double *d_alpha_own;              // ... handle-owned copy of a host schedule
    hipEvent_t sched_done;            // recorded behind the scheduling launches: a later launch on ANOTHER stream waits for it before it reads d_order
    hipStream_t sched_stream;         // the stream those launches ran on
    double *h_pack, *d_pack;          // small host-pointer batches (the reference's own scalar loop): inputs and outputs travel packed, one copy each way
    size_t pack_in, pack_out;         // doubles per instance in / out of the packed transfer
    const double *d_alpha;            // slack schedule in effect: d_alpha_own, a caller's device array, or null (the reference's formula)
    std::vector<hipEvent_t> ev_start, ev_stop;
    int ev_used;
    ncclComm_t comm;                  // RCCL communicator of the cost exchange (mpc_comm_init), or null
    int comm_rank, comm_world;
    double *d_gather_in, *d_gather_out;   // staging of the host-pointer all-gather
    size_t gather_cap;                // ... and its capacity in doubles of d_gather_in
    const double *d_yref;             // per-stage reference in effect (mpc_set_reference[_dev]): d_yref_own or a caller's device array; null = the goal's
    int32_t *d_ref_off;               // ... its row offsets (d_ref_off_own, a caller's device array, or null = 0)
    int ref_T;                        // ... rows per instance
    feature ref;
    double *d_yref_own;               // handle-owned copies of a host reference (mpc_set_reference)
    int32_t *d_ref_off_own;
    size_t yref_own_cap;              // ... capacity of d_yref_own in doubles
    feature ip;                       // per-instance parameters (mpc_set_instance_params[_dev]): mode 1, the tables below are final; mode 2, they are derived again from
                                      // the caller's arrays in front of every solve, on its stream
    ip_tables ip_own;                 // ... the tables of the caller's values, allocated on first use
    const double *ip_dev[4];          // ... mode 2: the caller's W, We, r_safe, r_hit (null = the handle's value)
    ip_tables ip_cfg;                 // ... the tables of the handle's own mpc_config values in every row: what the kernels from the masks' level on read without
                                      // instance parameters (ensure_companions; filled once, never written again)
    feature om;                       // per-instance obstacle masks (mpc_set_obstacle_mask[_dev]): host words are copied to d_omask_own
    const uint32_t *d_omask;          // ... the words the OSEL kernels read (KParams::omask)
    uint32_t *d_omask_own;            // ... handle-owned copy of host words, max_batch, allocated on first use
    feature bd;                       // per-instance box bounds (mpc_set_instance_bounds[_dev]): host arrays are packed into d_ip_b_own
    const double *d_ip_b;             // ... the packed table the IBND kernels read (KParams::ip_b), [.][kIpB]
    double *d_ip_b_own;               // ... handle-owned table of the host form, max_batch rows, allocated on first use
    uint32_t *d_omask_full;           // ... every obstacle present in max_batch words: what the IBND kernels (built on the masks' code) read without a mask
    int sqp_max;                      // SQP iterations per launch (mpc_set_sqp): <= 1 off
    double sqp_tol;                   // ... the step norm at or below which an instance stops
    int32_t *d_sqp_iters;             // ... the caller's words for the iterations run (mpc_set_sqp_iters_out_dev), or null
    double *d_ip_b_cfg;               // ... the handle's own bounds in max_batch rows: what the NSQP kernels (built on the bounds' code) read without instance bounds
    int32_t *d_refill_assign;         // mpc_episode_refill_dev: the per-slot assignment its deciding launch hands to its applying launch, max_batch words, allocated on first use
    bool rt_on;                       // per-seed tables / status log of the refill (mpc_set_refill_tables_dev): the caller's device pointers, used in place
    mpc_refill_tables rt;
    int ring_cap;                     // ring of seeded episodes (mpc_episode_ring_dev): entries, 0 = none attached; the caller's device arrays
    uint32_t *ring_state; double *ring_obst; int32_t *ring_tag, *ring_seed_src;
    bool ring_filled;                 // ... what the last mpc_episode_ring_fill_dev seeded it for: a refill with other values is refused
    int ring_scenario, ring_seed_count; unsigned ring_seed_first; double ring_box[6];
    int trace_rows, trace_max_steps;  // per-seed trajectories of a sweep (mpc_episode_trace_set_dev): rows, 0 = none attached; the caller's device arrays, used in place
    mpc_episode_trace trace;
    int grec_rows, grec_max_steps, grec_K;      // per-group record of multi-start episodes (mpc_group_record_set_dev): rows, 0 = none attached; the caller's device arrays
    mpc_group_record grec;
    int gg_mode;                      // guess family from geometry (mpc_set_guess_geometry): 0 off, 1 the amplitudes of seeded members from the obstacles in the way
    double gg_clearance, gg_a_max, gg_lead;
};

namespace {

// Row capacity of the kernel instantiation that runs a problem with n obstacles (NOBST of rti_solve_kernel / rti_split_kernel), and whether
// the problem leaves some of it unused (then only the mappings that take a run-time obstacle count are dispatched: the stage-split kernel for
// N <= 31, one instance per wavefront with row-parallel sweeps beyond).  20 and 32: the multi-wavefront kernel (rti_wide_kernel.hpp, N <= 31 only)
int row_capacity(int n) { return n <= 3 ? 3 : (n <= 5 ? 5 : (n <= 10 ? 10 : (n <= 20 ? 20 : 32))); }
constexpr int kMaxSplitN = 31;   // longest horizon of the two-lanes-per-stage mapping, hence of rti_wide_kernel
bool wide_rows(int n) { return n > 10; }
constexpr int kPackBatch = 64;   // host-pointer solves of at most this many instances use the packed transfer (solve_common)
bool partial_rows(const mpc_handle *h);
int feature_level(const mpc_handle *h);

mpc::KParams make_params(const mpc_config &c, int batch)
{
    mpc::KParams p;
    memset(&p, 0, sizeof(p));
    p.N = c.N; p.batch = batch; p.n_obst = c.n_obst;
    p.soft_h = c.soft_h; p.bx_terminal = c.bx_terminal; p.iter_max = c.qp_iter_max;
    p.dt = c.Tf / c.N; p.h2 = 0.5 * p.dt * p.dt;
    const double cs = c.cost_scale_dt ? p.dt : 1.0;
    const double lm = c.lm_scaled ? c.lm * p.dt : c.lm;
    // z order (ua, ual, x, y, psi, v, om); y = [x, y, v, om, ua, ual]  (robot_ocp_problem.py:64-68)
    p.Hd_stage[0] = cs * c.W[4] + lm; p.Hd_stage[1] = cs * c.W[5] + lm;
    p.Hd_stage[2] = cs * c.W[0] + lm; p.Hd_stage[3] = cs * c.W[1] + lm; p.Hd_stage[4] = lm;
    p.Hd_stage[5] = cs * c.W[2] + lm; p.Hd_stage[6] = cs * c.W[3] + lm;
    p.Hd_term[0] = c.We[0] + c.lm; p.Hd_term[1] = c.We[1] + c.lm; p.Hd_term[2] = c.lm;
    p.Hd_term[3] = c.We[2] + c.lm; p.Hd_term[4] = c.We[3] + c.lm;
    for (int k = 0; k < 6; k++) p.Wg[k] = cs * c.W[k];
    for (int k = 0; k < 4; k++) { p.Weg[k] = c.We[k]; p.bx_lo[k] = c.bx_lo[k]; p.bx_hi[k] = c.bx_hi[k]; }
    for (int k = 0; k < 2; k++) { p.bu_lo[k] = c.bu_lo[k]; p.bu_hi[k] = c.bu_hi[k]; }
    p.r2 = c.r_safe * c.r_safe;
    p.slack_a = c.slack_a; p.slack_b = c.slack_b; p.ss = c.slack_scale_dt ? p.dt : 1.0;
    p.tol = c.qp_tol; p.mu0 = c.mu0; p.thr0 = c.thr0;
    p.tl_min = mpc::kTLMin < 0.1 * c.qp_tol ? mpc::kTLMin : 0.1 * c.qp_tol;      // oracle/mpc_oracle.c tl_min()
    const bool truncate = c.qp_fail_policy == 1;      // oracle/mpc_oracle.c ipm_solve: the same three tests
    p.mu_div = truncate ? 1e300 : mpc::kMuDiverged * c.mu0;
    p.mu_cap = truncate ? INFINITY : mpc::kMuCapFailed * c.mu0;
    p.mu_settled = truncate ? INFINITY : c.mu0;
    p.polish_ratio = c.polish_ratio > 0.0 ? c.polish_ratio : INFINITY;      // off: c_max > inf * c_prev never holds (inf * 0 = NaN included)
    p.polish_tol = c.polish_tol > 0.0 ? (float)c.polish_tol : INFINITY;     // off: no estimate exceeds inf
    p.polish_tol_unsolved = c.polish_tol > 0.0 ? mpc::kPolishUnsolved * (float)c.polish_tol : INFINITY;
    p.polish_kappa = (float)c.polish_step_frac;
    p.polish_res_g = c.polish_res_g > 0.0 ? c.polish_res_g : INFINITY;      // off: ipm_head never asks for the residual
    return p;
}

mpc::World make_world(const mpc_config &c)
{
    mpc::World w;
    w.xmin = c.arena[0]; w.xmax = c.arena[1]; w.ymin = c.arena[2]; w.ymax = c.arena[3];
    w.bug_compat_predict = c.bug_compat_predict;
    return w;
}

int check_batch(mpc_handle *h, int batch)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (batch < 0 || batch > h->max_batch) return fail(MPC_ERR_ARG, "batch outside [0, max_batch]");
    return MPC_OK;
}

hipStream_t pick(mpc_handle *h, void *stream) { return stream ? (hipStream_t)stream : h->stream; }

// One owner for the handle's memory.  own: `count` elements of device (or pinned host) memory on first use -- a pointer that is set already is left
// alone -- recorded in the handle; disown: one of them given back early (a buffer that is regrown or switched off), its pointer nulled whatever the
// runtime answers; mpc_destroy releases what is still recorded.  There is no list of pointers to keep beside these.
template <class T> int own(mpc_handle *h, T **p, size_t count, bool pinned = false)
{
    if (*p) return MPC_OK;
    void *q = nullptr;
    h->owned.reserve(h->owned.size() + 1);
    HIPCHK(pinned ? hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, count * sizeof(T)));
    h->owned.push_back({q, pinned});
    *p = (T *)q;
    return MPC_OK;
}

hipError_t release(const owned_buf &b) { return b.pinned ? hipHostFree(b.p) : hipFree(b.p); }

template <class T> int disown(mpc_handle *h, T *&p)
{
    hipError_t e = hipSuccess;
    for (size_t k = 0; p && k < h->owned.size(); k++)
        if (h->owned[k].p == (void *)p) { e = release(h->owned[k]); h->owned.erase(h->owned.begin() + k); break; }
    p = nullptr;
    return e == hipSuccess ? MPC_OK : fail(MPC_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
}

// A host array into a buffer of the handle's (`cap` elements, allocated on first use), visible before the setter returns.  The wait in front of the
// copy: an earlier solve may still read the buffer
template <class T> int upload(mpc_handle *h, T **dst, size_t cap, const T *src, size_t n)
{
    int rc = own(h, dst, cap); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

// the kernel arguments of a solve: its inputs (the look-ahead P, or the obstacle states it is computed from inside the kernel) and outputs
mpc::KParams solve_params(mpc_handle *h, int batch, const double *x0, const double *P, const double *obst, const double *goal, double *X, double *U,
                          double *u0, double *cost, int32_t *status, int32_t *iters)
{
    mpc::KParams p = make_params(h->cfg, batch);
    p.x0 = x0; p.P = P; p.obst = obst; p.goal = goal; p.X = X; p.U = U;
    p.u0 = u0; p.cost = cost; p.status = status; p.iters = iters; p.trace = h->d_trace;
    if (obst) p.world = make_world(h->cfg);
    return p;
}

// Lanes per instance of the one-lane-per-stage mapping: the smallest of {16, 32, 64} with N + 1 < G (an idle lane separates instances that
// share a wavefront), or 21 -- three instances per wavefront on compact LDS blocks -- for 16 <= N <= 20 once pick_split hands a large batch
// to this mapping; unless overridden.  Packing instances into one wavefront multiplies throughput for large batches.
// (an obstacle mask is a run-time row count by nature: with one set, a handle whose count fills its capacity runs the run-time-count variants too;
// the instance bounds are built on the masks' code, so they do the same)
bool partial_rows(const mpc_handle *h) { return row_capacity(h->cfg.n_obst) != h->cfg.n_obst || feature_level(h) >= 3; }

int pick_lanes(mpc_handle *h, int batch)
{
    if (partial_rows(h)) return 64;
    const int need = h->cfg.N + 2;
    int G = need <= 16 ? 16 : (need <= 32 ? 32 : 64);
    // the matrix-core factorisation (opt-in, mpc_set_matrix_cores) maps one instance per wavefront; it is used for
    // batches of up to one instance per SIMD (1024 on MI355X), beyond that packing instances per wavefront wins
    if (batch <= 1024 && h->use_mfma) G = 64;
    if (h->lanes_override == 21) return 21;       // three instances per wavefront (N <= 20, row-parallel sweeps)
    // automatic: 17 <= N + 2 <= 22 (two instances per wavefront otherwise) with 3 or 5 obstacles, whenever pick_split leaves such a batch
    // to this mapping (more than 8 resp. 12 instances per SIMD)
    if (!h->lanes_override && !h->use_mfma && h->row_parallel && h->cfg.n_obst != 10 && need > 16 && h->cfg.N <= 20 &&
        batch > (h->cfg.n_obst == 3 ? 8 : 7) * h->simd_count) return 21;
    if (h->lanes_override >= G || (h->lanes_override && h->lanes_override >= need)) G = h->lanes_override;
    return G;
}

// Which lane mapping runs a batch (measured on MI355X, randomized C3-style workloads, closed loop, instance scheduling on;
// scripts/w2_probe.py -> profiles/r02_w2_probe_*.json; 10^6 solves/s: split 1 wavefront/SIMD | split 2 wavefronts/SIMD | one lane per stage
// with 2 (N = 20) or 4 (N = 10) instances per wavefront | with 3 instances per wavefront):
//                          batch 4096                  8192                       16384                      65536
//   N = 20,  3 obstacles:  7.0 | 6.1 | 5.5 | 5.4      9.7 | 10.1 |  9.8 |  9.7    10.6 | 12.6 | 16.0 | 16.0   11.3 | 14.0 | 20.7 | 20.7
//   N = 20,  5 obstacles:  7.1 | 5.5 | 5.3 | 5.2      8.5 |  7.8 |  8.4 |  9.0     9.3 |  9.2 | 12.9 | 13.0    9.7 | 10.0 | 16.1 | 16.1   (lean row state, new constants)
//   N = 20, 10 obstacles:  4.7 | 2.7 | 2.4 | 2.6      5.7 |  3.7 |  3.1 |  3.9     6.1 |  4.2 |  3.5 |  4.6    6.5 |  4.6 |  3.8 |  5.3
//   N = 31,  3 obstacles:  4.2 | 3.4 | 4.0 |  -       4.9 |  5.2 |  5.2 |  -       5.1 |  6.0 |  5.7 |  -      5.4 |  6.6 |  6.1 |  -
//   N = 10,  3 obstacles:  9.9 | 8.4 | 6.9 | 6.6     14.5 | 13.8 | 12.5 | 11.8    15.9 | 19.0 | 22.6 | 21.1   16.9 | 21.0 | 37.0 | 28.7
//   N = 10,  5 obstacles: 10.4 | 7.3 | 7.0 | 6.4     13.6 | 10.7 | 12.2 | 11.3    14.5 | 12.9 | 18.5 | 17.5   15.2 | 14.0 | 23.3 | 22.6   (lean row state, new constants)
// * the stage-split mapping (rows of a stage over 3 lanes for N <= 20, 2 for N <= 31, one instance per wavefront; rti_split_kernel.hpp) wins
//   up to ~8 instances per SIMD everywhere, and at every batch size with 10 obstacles (the one-lane row state spills) and for 20 < N <= 31;
// * beyond that the one-lane mappings that pack 3 (17 <= N + 2 <= 22) or 4 (N + 2 <= 16) instances into a wavefront win for 3 and 5
//   obstacles -- since instance scheduling (launch_solve) their wavefronts hold instances that stop together;
// * two wavefronts per SIMD (256 registers, compact LDS blocks) pay for 3 obstacles between ~4 and ~8 instances per SIMD and for
//   20 < N <= 31 beyond; with more obstacles the 256-register build spills 500 - 1150 bytes per lane and loses.
int pick_split(mpc_handle *h, int batch)
{
    if (wide_rows(h->cfg.n_obst)) return 2;       // rti_wide_kernel: two lanes per stage, whatever the batch
    const int N = h->cfg.N, no = row_capacity(h->cfg.n_obst);
    const int fit = N <= 20 ? 3 : (N <= 31 ? 2 : 1);
    if (partial_rows(h)) return (h->split_override > 1 && h->split_override <= fit) ? h->split_override : fit;
    if (h->use_mfma || !h->row_parallel || h->lanes_override) return 1;
    if (h->split_override) return h->split_override <= fit ? h->split_override : fit;
    if (no != 10 && N + 2 <= 16 && batch > 12 * h->simd_count) return 1;                      // four instances per wavefront (G = 16)
    if (no != 10 && N + 2 > 16 && N <= 20 && batch > (no == 3 ? 8 : 7) * h->simd_count) return 1;    // three instances per wavefront (G = 21)
    return fit;
}

int pick_waves(mpc_handle *h, int batch)
{
    if (partial_rows(h) || wide_rows(h->cfg.n_obst)) return 1;
    if (h->waves_override) return h->waves_override;
    return (h->cfg.n_obst == 3 && batch > 4 * h->simd_count) ? 2 : 1;
}

// More than 64 KB of dynamic LDS has to be granted per kernel function and device; the grant is remembered (largest size so far per
// kernel and device, beside the kernel's table row) instead of being re-issued on every launch.
constexpr int kMaxDevices = 64;
int g_granted[mpc::kSolveKernelCount][kMaxDevices];
int grant_lds(const mpc::KernelRow &row, int device, size_t lds)
{
    if (lds <= 65536) return MPC_OK;
    int (&granted)[kMaxDevices] = g_granted[&row - mpc::kSolveKernels];
    const int d = device < kMaxDevices ? device : kMaxDevices - 1;
    if (device < kMaxDevices && granted[d] >= (int)lds) return MPC_OK;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(row.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    granted[d] = (int)lds;
    return MPC_OK;
}

// Block-2 (partially condensed) stage recursions: the stage-split mapping on dense blocks, even horizons, all rows of the kernel's capacity in use
bool use_block2(const mpc_handle *h, bool w2, bool masked) { return h->block2 && !w2 && !masked && (h->cfg.N % 2 == 0) && h->cfg.N >= 4; }

// what rti_wide_kernel cannot run: horizons beyond two lanes per stage, and the mapping overrides that name a layout it does not have
int check_wide(const mpc_handle *h)
{
    if (h->cfg.N > kMaxSplitN) return fail(MPC_ERR_ARG, "more than 10 obstacles need N <= 31 (two lanes per horizon stage)");
    if (h->split_override != 0 && h->split_override != 2) return fail(MPC_ERR_ARG, "more than 10 obstacles run with two lanes per horizon stage only");
    if (h->lanes_override != 0 && h->lanes_override != 64) return fail(MPC_ERR_ARG, "more than 10 obstacles run with one instance per workgroup only");
    if (h->waves_override == 2) return fail(MPC_ERR_ARG, "more than 10 obstacles run with one wavefront per SIMD only");
    return MPC_OK;
}

// Per-stage reference (mpc_set_reference), feature level 1: the REF instantiations exist for the stage-split kernel (every horizon up to 31, at every batch
// size -- where the goal path would pack 3 or 4 instances into a wavefront the reference path stays on the split mapping), the multi-wavefront kernel,
// and one instance per wavefront on compact stage blocks (N > 31, or one lane per stage asked for).  The evidence mappings have none.
// Per-instance parameters (mpc_set_instance_params), level 2: the REF instantiations with one more flag, with or without a reference -- the same mappings,
// the same plan, the same refusals.
// Per-instance obstacle masks (mpc_set_obstacle_mask), level 3: the IPAR instantiations with a run-time row count and one more flag -- again the same
// mappings, plan and refusals; without instance parameters the tables they read hold the handle's own values
// Per-instance box bounds (mpc_set_instance_bounds), level 4: the OSEL instantiations with one more flag -- the same mappings, plan and refusals; without a
// mask they read words of the handle's own that have every obstacle present
// Several SQP iterations per launch (mpc_set_sqp), level 5: the IBND instantiations with one more flag -- the same mappings, plan and refusals; without
// instance bounds they read a table of the handle's own bounds
int feature_level(const mpc_handle *h) { return h->sqp_max > 1 ? 5 : (h->bd.mode ? 4 : (h->om.mode ? 3 : (h->ip.mode ? 2 : (h->ref.mode ? 1 : 0)))); }

int check_feature_mapping(const mpc_handle *h)
{
    const char *what[] = {"", "a per-stage reference", "per-instance parameters", "an obstacle mask", "instance bounds", "several SQP iterations per launch"};
    const char *w = what[feature_level(h)];
    if (h->use_mfma) return fail(MPC_ERR_ARG, "%s: no build for the matrix-core factorisation (mpc_set_matrix_cores)", w);
    if (!h->row_parallel) return fail(MPC_ERR_ARG, "%s: no build for the systolic sweeps (mpc_set_row_parallel(0))", w);
    if (h->block2) return fail(MPC_ERR_ARG, "%s: no build for the block-2 recursions (mpc_set_block_riccati)", w);
    if (h->lanes_override != 0 && h->lanes_override != 64) return fail(MPC_ERR_ARG, "%s: one instance per wavefront only (mpc_set_lanes_per_instance 0 or 64)", w);
    return MPC_OK;
}

// The lane mapping, kernel variant, launch geometry and dynamic-LDS size a batch runs with: the one place that decides them (launch_plan and
// mpc_get_kernel_name read it)
mpc::SolvePlan plan_solve(mpc_handle *h, int batch, bool lookahead)
{
    mpc::SolvePlan q = {};
    const int N = h->cfg.N, fit = N <= 20 ? 3 : (N <= 31 ? 2 : 1);
    q.cap = row_capacity(h->cfg.n_obst);
    q.masked = partial_rows(h);
    q.level = feature_level(h);
    q.lps = pick_split(h, batch);
    q.G = 64; q.fact = 3;
    q.grid = (unsigned)batch;
    // (the feature levels stay on the split mapping wherever the horizon fits it, unless one lane per stage is asked for)
    if (q.level && q.lps == 1 && fit > 1 && h->split_override != 1 && h->lanes_override != 64) q.lps = fit;
    if (wide_rows(h->cfg.n_obst)) {
        q.family = mpc::kWide;
    } else if (q.lps > 1) {
        q.family = mpc::kSplit;
        q.w2 = pick_waves(h, batch) == 2 && !q.masked;
        q.blk2 = !q.level && use_block2(h, q.w2, q.masked);
    } else if (!q.level) {
        q.G = pick_lanes(h, batch);
        const bool use_mfma = (q.G == 64) && h->use_mfma && !q.masked;
        const bool rowpar = (!use_mfma && h->row_parallel) || q.masked;
        // Compact stage blocks (look-ahead staged inside them): always with three instances per wavefront (13.5 KB per instance at N = 20:
        // four wavefronts of three per CU), and for long horizons on 64 lanes whenever the dense blocks would leave a CU fewer than the four
        // wavefronts its SIMDs can hold (N = 50, 10 obstacles: 51 KB -> 3 per CU dense, 32 KB -> 4 compact)
        const bool compact = rowpar && (q.G == 21 || (q.G == 64 && (mpc::one_lane_lds(q.cap, q.G, 2, N, lookahead) > 40960 || q.cap >= 10)));     // (ten row pairs: the compact kernel keeps its positions in LDS and has no scratch)
        q.fact = use_mfma ? 1 : (rowpar ? (compact ? 3 : 2) : 0);
        q.grid = (unsigned)((batch + 64 / q.G - 1) / (64 / q.G));
    }
    q.row = mpc::find_solve_kernel(q.key());
    if (q.row) { q.block = (unsigned)q.row->block; q.lds = q.row->lds(N, lookahead); }
    return q;
}

// What a plan's mapping refuses, decided here for the launch and for mpc_get_kernel_name alike
int check_plan(const mpc_handle *h, const mpc::SolvePlan &q)
{
    if (q.family == mpc::kWide) return check_wide(h);
    return q.level ? check_feature_mapping(h) : MPC_OK;
}

// launches the variant the plan names; no event handling here
int launch_plan(mpc_handle *h, const mpc::KParams &p, hipStream_t s, const mpc::SolvePlan &q)
{
    int rc = check_plan(h, q); if (rc) return rc;
    if (!q.row) {
        if (q.family != mpc::kOneLane) return fail(MPC_ERR_ARG, "n_obst must be in [1, 10]");
        if (q.masked) return fail(MPC_ERR_ARG, "no kernel variant for this lane mapping with n_obst outside {3, 5, 10}");
        return fail(MPC_ERR_ARG, "no kernel variant for this lane mapping (three instances per wavefront need the row-parallel sweeps)");
    }
    rc = grant_lds(*q.row, h->device, q.lds); if (rc) return rc;
    hipLaunchKernelGGL(q.row->fn, dim3(q.grid), dim3(q.block), q.lds, s, p);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int create_resources(mpc_handle *h)
{
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->device));
    h->simd_count = 4 * prop.multiProcessorCount;
    const size_t B = (size_t)h->max_batch, N = (size_t)h->cfg.N, no = (size_t)h->cfg.n_obst;
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->pack_in = 5 + 2 + (N + 1) * no * 2;      // x0 | goal | P (or the 4 n_obst obstacle states, which are fewer)
    h->pack_out = 2 + 1 + 1;                    // u0 | cost | status, iters (two int32 in one double's space)
    const size_t pack = (size_t)kPackBatch * (h->pack_in + h->pack_out);
    int rc = MPC_OK;
    auto get = [&](auto **p, size_t count, bool pinned = false) { if (!rc) rc = own(h, p, count, pinned); };      // (nothing more once one has failed)
    get(&h->dX, B * (N + 1) * 5); get(&h->dU, B * N * 2);
    get(&h->d_x0, B * 5); get(&h->d_P, B * (N + 1) * no * 2); get(&h->d_goal, B * 2); get(&h->d_obst, B * no * 4);
    get(&h->d_u0, B * 2); get(&h->d_cost, B); get(&h->d_status, B); get(&h->d_iters, B);
    get(&h->d_xa, B * 5); get(&h->d_ua, B * 2); get(&h->d_xb, B * 5);
    get(&h->d_order, B); get(&h->d_iters_sched, B);
    get(&h->d_sched_hist, (size_t)mpc::kSchedBins * ((B + mpc::kSchedChunk - 1) / mpc::kSchedChunk));
    get(&h->h_pack, pack, true); get(&h->d_pack, pack);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->d_iters_sched, 0, B * sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->dX, 0, B * (N + 1) * 5 * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(h->dU, 0, B * N * 2 * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int launch_schedule(mpc_handle *h, int batch, const int32_t *d_iters, hipStream_t s)
{
    const int nblk = (batch + mpc::kSchedChunk - 1) / mpc::kSchedChunk;
    hipLaunchKernelGGL(mpc::schedule_count_kernel, dim3(nblk), dim3(mpc::kSchedThreads), 0, s, batch, nblk, d_iters, h->d_sched_hist);
    hipLaunchKernelGGL(mpc::schedule_scatter_kernel, dim3(nblk), dim3(mpc::kSchedThreads), 0, s, batch, nblk, d_iters, h->d_sched_hist, h->d_order);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// The derived per-instance tables (KParams::ip_w, ip_r2, ip_rhit) from the W, We, r_safe, r_hit in effect -- a null group takes the handle's mpc_config value.
// ONE definition of every derived value for the host and the device (instance_params_kernel): each product and sum is a separately rounded operation,
// as make_params forms Hd_stage, Hd_term, Wg, Weg and r2 on the host, so a batch that repeats the handle's own values reproduces the handle path bit for bit
mpc::IpDefaults ip_from_config(const mpc_config &c)
{
    mpc::IpDefaults d;
    const double dt = c.Tf / c.N;
    d.cs = c.cost_scale_dt ? dt : 1.0;
    d.lm_stage = c.lm_scaled ? c.lm * dt : c.lm;
    d.lm_term = c.lm;
    for (int k = 0; k < 6; k++) d.W[k] = c.W[k];
    for (int k = 0; k < 4; k++) d.We[k] = c.We[k];
    d.r_safe = c.r_safe;
    d.r_hit = 1.0 + 0.2;               // o.r + R_ROBOT, as mpc_closed_loop_step_dev sets it
    d.hit_off = c.r_safe - d.r_hit;    // r_safe given, r_hit not: r_hit[b][j] = r_safe[b][j] - (cfg.r_safe - 1.2), the handle's margin between the two radii
    return d;
}

// The derived tables of `rows` instances from host arrays (a null group: the handle's value) into one set of the handle's tables
int upload_instance_tables(mpc_handle *h, ip_tables &t, int rows, const double *W, const double *We, const double *r_safe, const double *r_hit)
{
    const size_t B = (size_t)h->max_batch, R = (size_t)rows, no = (size_t)h->cfg.n_obst;
    const mpc::IpDefaults d = ip_from_config(h->cfg);
    std::vector<double> tw(R * mpc::kIpW), t2(R * no), th(R * no);
    for (int b = 0; b < rows; b++)
        mpc::derive_instance_params(d, b, (int)no, W, We, r_safe, r_hit, tw.data(), t2.data(), th.data());
    int rc = upload(h, &t.w, B * mpc::kIpW, tw.data(), tw.size());
    if (!rc) rc = upload(h, &t.r2, B * no, t2.data(), t2.size());
    if (!rc) rc = upload(h, &t.rhit, B * no, th.data(), th.size());
    return rc;
}

uint32_t all_obstacles(const mpc_handle *h) { return h->cfg.n_obst >= 32 ? 0xffffffffu : ((1u << h->cfg.n_obst) - 1u); }

// The packed bounds table of the IBND kernels, max_batch rows: the first `batch` from the host arrays (a null group: the handle's value), validated; the
// rows behind them hold the handle's own values (no solve reads them).  batch 0: the handle's own bounds in every row
int pack_bounds(const mpc_handle *h, int batch, const double *bx_lo, const double *bx_hi, const double *bu_lo, const double *bu_hi, std::vector<double> &tab)
{
    struct Group { const char *lo_name, *hi_name; const double *lo, *hi, *cfg_lo, *cfg_hi; int n, lo_at, hi_at; };
    const Group groups[2] = {{"bu_lo", "bu_hi", bu_lo, bu_hi, h->cfg.bu_lo, h->cfg.bu_hi, 2, mpc::kIpBuLo, mpc::kIpBuHi},
                             {"bx_lo", "bx_hi", bx_lo, bx_hi, h->cfg.bx_lo, h->cfg.bx_hi, 4, mpc::kIpBxLo, mpc::kIpBxHi}};
    tab.resize((size_t)h->max_batch * mpc::kIpB);
    for (const Group &g : groups) {
        for (size_t k = 0; k < (size_t)batch * g.n; k++) {
            if (g.lo && !(g.lo[k] >= -1e300 && g.lo[k] <= 1e300)) return fail(MPC_ERR_ARG, "instance bounds: %s entries must be finite", g.lo_name);
            if (g.hi && !(g.hi[k] >= -1e300 && g.hi[k] <= 1e300)) return fail(MPC_ERR_ARG, "instance bounds: %s entries must be finite", g.hi_name);
        }
        for (int b = 0; b < h->max_batch; b++)
            for (int k = 0; k < g.n; k++) {
                const double lo = (g.lo && b < batch) ? g.lo[(size_t)b * g.n + k] : g.cfg_lo[k], hi = (g.hi && b < batch) ? g.hi[(size_t)b * g.n + k] : g.cfg_hi[k];
                if (b < batch && !(lo < hi)) return fail(MPC_ERR_ARG, "instance bounds: %s must be below %s in every component", g.lo_name, g.hi_name);
                tab[(size_t)b * mpc::kIpB + g.lo_at + k] = lo; tab[(size_t)b * mpc::kIpB + g.hi_at + k] = hi;
            }
    }
    return MPC_OK;
}

// Companions: what the kernels of a feature level read for the features below it that the caller has not set -- from the masks' level (3) on the instance
// tables of the handle's own values, from the bounds' (4) a mask with every obstacle present, at the SQP loop's (5) a table of the handle's own bounds.
// Each lives in a buffer of its own, is filled once and never written again, so switching a feature below off needs no refill.  Host calls (they wait for
// the handle's stream): made by the setters that raise the level (mask, bounds, SQP) in front of their state change, never in front of a solve
int ensure_companions(mpc_handle *h, int level)
{
    const size_t B = (size_t)h->max_batch;
    int rc = MPC_OK;
    if (level >= 3 && !h->ip_cfg.rhit) rc = upload_instance_tables(h, h->ip_cfg, h->max_batch, nullptr, nullptr, nullptr, nullptr);      // (rhit: the last it fills)
    if (!rc && level >= 4 && !h->d_omask_full) {
        const std::vector<uint32_t> full(B, all_obstacles(h));
        rc = upload(h, &h->d_omask_full, B, full.data(), B);
    }
    if (!rc && level >= 5 && !h->d_ip_b_cfg) {
        std::vector<double> tab;
        rc = pack_bounds(h, 0, nullptr, nullptr, nullptr, nullptr, tab);
        if (!rc) rc = upload(h, &h->d_ip_b_cfg, tab.size(), tab.data(), tab.size());
    }
    return rc;
}

// a feature that is on covers the batch, or the launch is refused with the feature's own sentence
int check_covered(const feature &f, int batch, const char *refusal) { return f.mode && batch > f.batch ? fail(MPC_ERR_ARG, "%s", refusal) : MPC_OK; }

// In front of a launch that reads them: the coverage checks and kernel arguments of the per-stage reference, the per-instance tables (derived here from
// device arrays, mode 2) and, for a solve, of what its feature level reads beside them -- the caller's where a feature is set, the handle's companion
// (ensure_companions) where it is not -- and the slack schedule
enum AttachFor { kForSolve, kForLinearize };
int attach_inputs(mpc_handle *h, mpc::KParams &p, hipStream_t s, AttachFor what)
{
    const bool solve = what == kForSolve;
    const int level = solve ? feature_level(h) : 0;
    p.yref = h->d_yref; p.ref_off = h->d_ref_off; p.ref_T = h->ref_T;
    int rc = check_covered(h->ref, p.batch, solve ? "the per-stage reference set by mpc_set_reference covers fewer instances than this solve"
                                                  : "the per-stage reference set by mpc_set_reference covers fewer instances than this call");
    if (rc) return rc;
    if ((p.fused & MPC_STEP_ADVANCE_REF) && (!h->d_yref || !h->d_ref_off))
        return fail(MPC_ERR_ARG, "MPC_STEP_ADVANCE_REF needs a per-stage reference with offsets (mpc_set_reference[_dev])");
    rc = check_covered(h->ip, p.batch, "the per-instance parameters set by mpc_set_instance_params cover fewer instances than this solve"); if (rc) return rc;
    if (h->ip.mode == 2) {
        hipLaunchKernelGGL(mpc::instance_params_kernel, dim3((p.batch + 127) / 128), dim3(128), 0, s, ip_from_config(h->cfg), p.batch, h->cfg.n_obst,
                           h->ip_dev[0], h->ip_dev[1], h->ip_dev[2], h->ip_dev[3], h->ip_own.w, h->ip_own.r2, h->ip_own.rhit);
        HIPCHK(hipGetLastError());
    }
    const ip_tables &t = h->ip.mode ? h->ip_own : h->ip_cfg;
    if (h->ip.mode || level >= 3) { p.ip_w = t.w; p.ip_r2 = t.r2; p.ip_rhit = t.rhit; }
    if (!solve) return MPC_OK;
    rc = check_covered(h->om, p.batch, "the obstacle mask set by mpc_set_obstacle_mask covers fewer instances than this solve"); if (rc) return rc;
    if (level >= 3) p.omask = h->om.mode ? h->d_omask : h->d_omask_full;
    rc = check_covered(h->bd, p.batch, "the instance bounds set by mpc_set_instance_bounds cover fewer instances than this solve"); if (rc) return rc;
    if (level >= 4) p.ip_b = h->bd.mode ? h->d_ip_b : h->d_ip_b_cfg;
    if (level == 5) { p.sqp_max = h->sqp_max; p.sqp_tol = h->sqp_tol; p.sqp_iters = h->d_sqp_iters; }
    // an uploaded schedule covers the instances it was uploaded for: rows behind them were never written (the kernels index alpha[inst][i])
    p.alpha = h->d_alpha;
    return check_covered(h->alpha, p.batch, "the slack schedule set by mpc_set_slack_schedule covers fewer instances than this solve");
}

// For a launch that stands beside the solve of `batch` instances (geometry guesses, group step, group refill, rollout merit): that solve's kernel arguments
// as it would be launched now -- its constants, the inputs given, its per-instance tables with their coverage checks (attach; false: constants and inputs
// alone, nothing is checked) --, none of its outputs, no trace
int beside_solve(mpc_handle *h, int batch, const double *x0, const double *P, const double *goal, hipStream_t s, bool attach, mpc::KParams &p)
{
    p = solve_params(h, batch, x0, P, nullptr, goal, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    p.trace = nullptr;
    return attach ? attach_inputs(h, p, s, kForSolve) : MPC_OK;
}

int launch_solve(mpc_handle *h, mpc::KParams &p, hipStream_t s)
{
    p.iters_acc = h->d_iters_acc; p.status_acc = h->d_status_acc;
    int rc_in = attach_inputs(h, p, s, kForSolve); if (rc_in) return rc_in;
    const mpc::SolvePlan q = plan_solve(h, p.batch, p.obst != nullptr);
    // Instance scheduling (aux_kernels.hpp::schedule_kernel): wavefront slots are dealt the instances in the order of their iteration counts
    // in this handle's previous launch of the same batch size, longest first -- instances that share a wavefront then stop together, and
    // the rare 50-iteration instance starts in the first round of wavefronts instead of stretching the last one; the order for the NEXT
    // launch is rebuilt behind this one, on the same stream.  A batch of at most one wavefront per SIMD has nothing to gain from it.
    const bool sched = h->scheduling && p.batch > h->simd_count;
    p.order = (sched && h->order_batch == p.batch) ? h->d_order : nullptr;
    if (sched && !p.iters) p.iters = h->d_iters_sched;
    // the order, its histograms and d_iters_sched belong to the handle but the launches go to the caller's stream: a launch on a different stream
    // than the one that built them must not start (nor rebuild them) while that one is still writing
    if (sched && h->sched_done && h->order_batch && h->sched_stream != s) HIPCHK(hipStreamWaitEvent(s, h->sched_done, 0));
    // profiling: a start / stop event pair from the pool (created by mpc_profile_enable, never here) around every k-th launch; the pair
    // counts only when both records and the launch between them succeeded
    const bool timed = h->profiling && (h->launch_count++ % h->profiling) == 0 && h->ev_used < (int)h->ev_start.size();
    if (timed) HIPCHK(hipEventRecord(h->ev_start[h->ev_used], s));
    int rc = launch_plan(h, p, s, q);
    if (rc) return rc;
    if (timed) {
        HIPCHK(hipEventRecord(h->ev_stop[h->ev_used], s));
        h->ev_used++;
    }
    if (sched) {
        h->order_batch = 0;
        rc = launch_schedule(h, p.batch, p.iters, s); if (rc) return rc;
        if (!h->sched_done) HIPCHK(hipEventCreateWithFlags(&h->sched_done, hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->sched_done, s));
        h->sched_stream = s;
        h->order_batch = p.batch;
    }
    return MPC_OK;
}

}  // namespace

extern "C" {

const char *mpc_last_error(void) { return g_err; }

int mpc_abi_version(void) { return MPC_ABI_VERSION; }

int mpc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mpc_default_config(mpc_config *c, int N, int n_obst, double Tf)
{
    if (!c) return fail(MPC_ERR_ARG, "null config");
    memset(c, 0, sizeof(*c));
    c->N = N; c->n_obst = n_obst; c->Tf = Tf;
    for (int k = 0; k < 4; k++) { c->W[k] = 2.0; c->We[k] = 5.0; }   // robot_ocp_problem.py:24-27
    c->W[4] = c->W[5] = 0.15;
    c->lm = 2.0;                                                       // :128
    c->bx_lo[0] = c->bx_lo[1] = -7.0; c->bx_hi[0] = c->bx_hi[1] = 7.0;      // :91-92
    c->bx_lo[2] = c->bx_lo[3] = -10.0; c->bx_hi[2] = c->bx_hi[3] = 10.0;
    c->bu_lo[0] = c->bu_lo[1] = -8.0; c->bu_hi[0] = c->bu_hi[1] = 8.0;      // :95-96
    c->r_safe = 1.0 + 0.2 + 1.2;                                       // robot_model.py:62
    c->slack_a = 1e4; c->slack_b = 50.0;                               // :146
    c->qp_iter_max = 50;                                               // world_specification.py:48
    c->qp_tol = 1e-10;
    c->cost_scale_dt = 1; c->slack_scale_dt = 1; c->lm_scaled = 1; c->bx_terminal = 0; c->soft_h = 1;   // the switch set that replays the reference's recorded tables per seed (profiles/r02_seed_replay.json)
    c->arena[0] = -8.0; c->arena[1] = 8.0; c->arena[2] = -8.0; c->arena[3] = 8.0;   // world_specification.py:7-10
    c->bug_compat_predict = 1;
    c->mu0 = 1e4;
    /* thr0: 0.1; from 8 obstacles on 0.3 (round 4, scripts/thr0_probe.py: -4 % iterations and +5 % solves/s on C5's problem, +2.6 % at N = 20 with 10 obstacles).  0.3 would
     * also gain 3 % at C2 and 1 % at C3 and reproduce 420 instead of 416 recorded rows, but one of the 41 seeds on which the recorded tables prove that acados converged
     * within 25 iterations then needs more than 25 here (profiles/r04_thr0_probe.txt): the reference's own problem size keeps the constant its pin was made with. */
    c->thr0 = n_obst >= 8 ? 0.3 : 0.1;
    c->qp_fail_policy = 0;
    c->polish_ratio = 1e-2; c->polish_tol = 1e-6;      // oracle/mpc_oracle.c orc_default_config
    c->polish_step_frac = N >= 30 ? 0.01 : 0.0;         // ... which says why the horizon is in this default
    c->polish_res_g = 1e-7;
    return MPC_OK;
}

// mpc_create (1 .. 10 obstacles) and mpc_create2 (1 .. MPC_MAX_OBST; beyond 10 with N <= 31): one validation, one construction
static int create_handle(const mpc_config *cfg, int device, int max_batch, mpc_handle **out, int max_obst)
{
    if (!cfg || !out) return fail(MPC_ERR_ARG, "null argument");
    if (cfg->N < 2 || cfg->N > 62) return fail(MPC_ERR_ARG, "N must be in [2, 62] (one horizon stage per lane, N + 1 < 64)");
    if (cfg->n_obst < 1 || cfg->n_obst > max_obst) return fail(MPC_ERR_ARG, max_obst == 10 ? "n_obst must be in [1, 10]" : "n_obst must be in [1, 32]");
    if (wide_rows(cfg->n_obst) && cfg->N > kMaxSplitN) return fail(MPC_ERR_ARG, "more than 10 obstacles need N <= 31 (two lanes per horizon stage)");
    if (max_batch < 1) return fail(MPC_ERR_ARG, "max_batch must be >= 1");
    if (!(cfg->Tf > 0) || !(cfg->qp_tol > 0) || cfg->qp_iter_max < 1) return fail(MPC_ERR_ARG, "Tf, qp_tol, qp_iter_max must be positive");
    if (cfg->qp_fail_policy != 0 && cfg->qp_fail_policy != 1) return fail(MPC_ERR_ARG, "qp_fail_policy must be 0 (divergence tests) or 1 (truncate at qp_iter_max)");
    if (!(cfg->polish_ratio >= 0.0) || !(cfg->polish_ratio <= 1.0)) return fail(MPC_ERR_ARG, "polish_ratio must be in [0, 1] (0 = that indicator off)");
    if (!(cfg->polish_tol >= 0.0) || !(cfg->polish_tol <= 1.0)) return fail(MPC_ERR_ARG, "polish_tol must be in [0, 1] (0 = that indicator off)");
    if (!(cfg->polish_step_frac >= 0.0) || !(cfg->polish_step_frac <= 0.5)) return fail(MPC_ERR_ARG, "polish_step_frac must be in [0, 0.5]");
    if (!(cfg->polish_res_g >= 0.0)) return fail(MPC_ERR_ARG, "polish_res_g must be >= 0 (0 = that indicator off)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPC_ERR_NODEVICE, "no HIP device visible: libmpcgpu has no CPU path");
    if (device < 0 || device >= ndev) return fail(MPC_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    mpc_handle *h = new mpc_handle();     // value-initialised: every pointer null, so mpc_destroy can release a half-built handle
    h->cfg = *cfg; h->device = device; h->max_batch = max_batch;
    h->row_parallel = 1; h->scheduling = 1; h->block2 = 0;      // block-2 recursions: built, parity-tested, measured 5 % slower at C2 -> opt-in
    int rc = create_resources(h);
    if (rc) { mpc_destroy(h); return rc; }     // (mpc_destroy leaves g_err alone when nothing fails inside it)
    *out = h;
    return MPC_OK;
}

int mpc_create(const mpc_config *cfg, int device, int max_batch, mpc_handle **out) { return create_handle(cfg, device, max_batch, out, 10); }

int mpc_create2(const mpc_config *cfg, int device, int max_batch, mpc_handle **out) { return create_handle(cfg, device, max_batch, out, MPC_MAX_OBST); }

int mpc_destroy(mpc_handle *h)
{
    if (!h) return MPC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto e : h->ev_start) (void)hipEventDestroy(e);
    for (auto e : h->ev_stop) (void)hipEventDestroy(e);
    if (h->sched_done) (void)hipEventDestroy(h->sched_done);
    (void)mpc_comm_destroy(h);
    for (const owned_buf &b : h->owned) (void)release(b);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return MPC_OK;
}

int mpc_iterate_ptrs(mpc_handle *h, double **d_X, double **d_U, void **stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (d_X) *d_X = h->dX;
    if (d_U) *d_U = h->dU;
    if (stream) *stream = (void *)h->stream;
    return MPC_OK;
}

/* ------------------------------------------------ device-pointer API ------------------------------------------------ */

int mpc_solve_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_P, const double *d_goal,
                  double *d_X, double *d_U, double *d_u0, double *d_cost, int32_t *d_status, int32_t *d_iters, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_x0 || !d_P || !d_goal || !d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    mpc::KParams p = solve_params(h, batch, d_x0, d_P, nullptr, d_goal, d_X, d_U, d_u0, d_cost, d_status, d_iters);
    return launch_solve(h, p, pick(h, stream));
}

int mpc_closed_loop_step_dev(mpc_handle *h, int batch, double *d_x0, double *d_obst, const double *d_goal, double *d_X, double *d_U,
                             double *d_u0, double *d_cost, int32_t *d_status, int32_t *d_iters, const double *d_noise,
                             double randomness, double vmax, int flags, double *d_min_margin, int32_t *d_ep_flags, int32_t *d_ep_steps,
                             void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_x0 || !d_obst || !d_goal || !d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer");
    if ((flags & MPC_STEP_METRICS) && (!d_min_margin || !d_ep_flags || !d_ep_steps)) return fail(MPC_ERR_ARG, "metrics requested without buffers");
    HIPCHK(hipSetDevice(h->device));
    mpc::KParams p = solve_params(h, batch, d_x0, nullptr, d_obst, d_goal, d_X, d_U, d_u0, d_cost, d_status, d_iters);
    p.x0_rw = d_x0; p.obst_rw = d_obst; p.noise = d_noise;
    p.randomness = randomness; p.vmax = vmax;
    p.tol_goal = 0.15;               // TOL, src/models/world_specification.py:45
    p.r_hit = 1.0 + 0.2;             // o.r + R_ROBOT, robot_ocp_problem.py:224
    p.fused = flags;
    p.ep_min_margin = d_min_margin; p.ep_flags = d_ep_flags; p.ep_steps = d_ep_steps;
    return launch_solve(h, p, pick(h, stream));
}

int mpc_predict_dev(mpc_handle *h, int batch, const double *d_obst, double *d_P, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_obst || !d_P) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    const int count = batch * h->cfg.n_obst;
    hipLaunchKernelGGL(mpc::predict_kernel, dim3((count + 255) / 256), dim3(256), 0, pick(h, stream), make_world(h->cfg), count,
                       h->cfg.n_obst, h->cfg.N, h->cfg.Tf / h->cfg.N, d_obst, d_P);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_shift_dev(mpc_handle *h, int batch, double *d_X, double *d_U, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::shift_kernel, dim3(batch), dim3(64), 0, pick(h, stream), batch, h->cfg.N, d_X, d_U);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

static int reset_guess_launch(mpc_handle *h, int batch, const double *d_x0, const double *d_goal, double *d_X, double *d_U, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_x0 || !d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    const int count = batch * (h->cfg.N + 1);
    hipLaunchKernelGGL(mpc::reset_guess_kernel, dim3((count + 255) / 256), dim3(256), 0, pick(h, stream), batch, h->cfg.N, d_x0, d_goal, d_X, d_U);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_reset_guess_dev(mpc_handle *h, int batch, const double *d_x0, double *d_X, double *d_U, void *stream)
{
    return reset_guess_launch(h, batch, d_x0, nullptr, d_X, d_U, stream);
}

int mpc_reset_guess_interp_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_goal, double *d_X, double *d_U, void *stream)
{
    if (!d_goal) return fail(MPC_ERR_ARG, "null device pointer");
    return reset_guess_launch(h, batch, d_x0, d_goal, d_X, d_U, stream);
}

// the group layout of the two multi-start entry points: `groups` scenarios of K members, member k of group g = instance g K + k
static_assert(mpc::kSelectBroadcast == MPC_SELECT_BROADCAST, "the kernel's flag is the header's");
static int check_groups(mpc_handle *h, int groups, int K)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (K < 1 || K > 64) return fail(MPC_ERR_ARG, "K must be in [1, 64] (one member per lane of the group's wavefront)");
    if (groups < 0 || (long long)groups * K > h->max_batch) return fail(MPC_ERR_ARG, "groups * K outside [0, max_batch]");
    return MPC_OK;
}

int mpc_seed_guesses_dev(mpc_handle *h, int groups, int K, const double *d_x0, const double *d_goal, const double *d_offsets, int keep_first,
                         double *d_X, double *d_U, void *stream)
{
    int rc = check_groups(h, groups, K); if (rc) return rc;
    if (groups == 0) return MPC_OK;
    if (!d_x0 || !d_goal || !d_offsets || !d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    const int count = groups * K;
    hipLaunchKernelGGL(mpc::seed_guesses_kernel, dim3((count + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, pick(h, stream),
                       groups, K, h->cfg.N, keep_first ? 1 : 0, d_x0, d_goal, d_offsets, d_X, d_U);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_set_guess_geometry(mpc_handle *h, int mode, double clearance, double a_max, double lead)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (mode != 0 && mode != 1) return fail(MPC_ERR_ARG, "mpc_set_guess_geometry: mode must be 0 (off) or 1 (amplitudes from the obstacle geometry)");
    if (!(clearance >= 0.0) || !std::isfinite(clearance)) return fail(MPC_ERR_ARG, "mpc_set_guess_geometry: clearance must be finite and >= 0");
    if (!(a_max > 0.0) || !std::isfinite(a_max)) return fail(MPC_ERR_ARG, "mpc_set_guess_geometry: a_max must be finite and > 0");
    if (!(lead >= 0.0) || !std::isfinite(lead)) return fail(MPC_ERR_ARG, "mpc_set_guess_geometry: lead must be finite and >= 0");
    h->gg_mode = mode; h->gg_clearance = clearance; h->gg_a_max = a_max; h->gg_lead = lead;
    return MPC_OK;
}

// the rule's parameters and the tables it reads of a solve over `p.batch` instances (attach_inputs has filled p): the r_safe^2 rows and the mask, or null
static mpc::GuessGeom guess_geom(const mpc_handle *h, const mpc::KParams &p)
{
    mpc::GuessGeom q;
    q.mode = h->gg_mode; q.clearance = h->gg_clearance; q.a_max = h->gg_a_max; q.lead = h->gg_lead;
    q.r_safe = h->cfg.r_safe; q.ip_r2 = p.ip_r2; q.omask = p.omask;
    return q;
}

int mpc_seed_guesses_geom_dev(mpc_handle *h, int groups, int K, const double *d_x0, const double *d_obst, const double *d_goal, const double *d_offsets,
                              int keep_first, double *d_X, double *d_U, double *d_offsets_out, void *stream)
{
    int rc = check_groups(h, groups, K); if (rc) return rc;
    if (!h->gg_mode) return fail(MPC_ERR_ARG, "mpc_seed_guesses_geom_dev: the guess geometry is off (mpc_set_guess_geometry); mpc_seed_guesses_dev seeds the fixed family");
    if (groups == 0) return MPC_OK;
    if (!d_x0 || !d_obst || !d_goal || !d_offsets || !d_X || !d_U) return fail(MPC_ERR_ARG, "null device pointer (only d_offsets_out may be null)");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick(h, stream);
    const int count = groups * K;
    // the per-instance tables of the solve the guesses are for (r_safe rows, obstacle mask), with that solve's coverage checks
    mpc::KParams p;
    rc = beside_solve(h, count, nullptr, nullptr, nullptr, s, true, p); if (rc) return rc;
    hipLaunchKernelGGL(mpc::seed_guesses_geom_kernel, dim3((count + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, s,
                       guess_geom(h, p), groups, K, h->cfg.N, h->cfg.n_obst, keep_first ? 1 : 0, d_x0, d_obst, d_goal, d_offsets, d_X, d_U, d_offsets_out);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_select_best_dev(mpc_handle *h, int groups, int K, const double *d_cost, const int32_t *d_status, double incumbent_margin, int flags,
                        double *d_X, double *d_U, int32_t *d_winner, double *d_best_cost, double *d_best_u0, const double *d_u0, void *stream)
{
    int rc = check_groups(h, groups, K); if (rc) return rc;
    if (!(incumbent_margin >= 0.0) || !(incumbent_margin < 1.0)) return fail(MPC_ERR_ARG, "incumbent_margin must be in [0, 1)");
    if (flags & ~MPC_SELECT_BROADCAST) return fail(MPC_ERR_ARG, "unknown flags (MPC_SELECT_BROADCAST is the only one)");
    if (groups == 0) return MPC_OK;
    if (!d_cost || !d_status || !d_winner) return fail(MPC_ERR_ARG, "null device pointer (d_cost, d_status and d_winner are mandatory)");
    if ((flags & MPC_SELECT_BROADCAST) && (!d_X || !d_U)) return fail(MPC_ERR_ARG, "MPC_SELECT_BROADCAST needs d_X and d_U");
    if (d_best_u0 && !d_u0 && !d_U) return fail(MPC_ERR_ARG, "d_best_u0 needs d_u0 or d_U");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::select_best_kernel, dim3((groups + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, pick(h, stream),
                       groups, K, h->cfg.N, incumbent_margin, flags, d_cost, d_status, d_X, d_U, d_winner, d_best_cost, d_best_u0, d_u0);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

static_assert(mpc::kGroupMarginAll == MPC_GROUP_MARGIN_ALL, "the kernel's flag is the header's");
int mpc_group_step_dev(mpc_handle *h, int groups, int K, const double *d_key, const int32_t *d_status, const double *d_u0, double incumbent_margin,
                       int flags, double *d_x, double *d_obst, const double *d_goal, const double *d_offsets, const double *d_noise, double randomness,
                       double vmax, double *d_X, double *d_U, const mpc_group_step_out *out, void *stream)
{
    int rc = check_groups(h, groups, K); if (rc) return rc;
    if (!(incumbent_margin >= 0.0) || !(incumbent_margin < 1.0)) return fail(MPC_ERR_ARG, "incumbent_margin must be in [0, 1)");
    if (flags & ~MPC_GROUP_MARGIN_ALL) return fail(MPC_ERR_ARG, "unknown flags (MPC_GROUP_MARGIN_ALL is the only one)");
    if (groups == 0) return MPC_OK;
    if (!d_key || !d_status || !d_u0 || !d_x || !d_obst || !d_goal || !d_offsets || !d_X || !d_U || !out)
        return fail(MPC_ERR_ARG, "null device pointer (d_key, d_status, d_u0, d_x, d_obst, d_goal, d_offsets, d_X, d_U and out are mandatory)");
    if (!out->winner || !out->min_margin || !out->ep_flags || !out->ep_steps)
        return fail(MPC_ERR_ARG, "null device pointer in out (winner, min_margin, ep_flags and ep_steps are mandatory)");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick(h, stream);
    // the per-instance tables of the solve this step stands behind (r_hit rows, obstacle mask), with that solve's coverage checks
    mpc::KParams p;
    rc = beside_solve(h, groups * K, nullptr, nullptr, nullptr, s, true, p); if (rc) return rc;
    mpc::GroupStepArgs a;
    a.groups = groups; a.K = K; a.N = h->cfg.N; a.n_obst = h->cfg.n_obst; a.flags = flags;
    a.margin = incumbent_margin; a.dt = h->cfg.Tf / h->cfg.N; a.randomness = randomness; a.vmax = vmax;
    a.tol_goal = 0.15;               // TOL, src/models/world_specification.py:45
    a.r_hit = 1.0 + 0.2;             // o.r + R_ROBOT, as mpc_closed_loop_step_dev sets it
    a.world = make_world(h->cfg);
    a.key = d_key; a.status = d_status; a.u0 = d_u0; a.goal = d_goal; a.offsets = d_offsets; a.noise = d_noise;
    a.x = d_x; a.obst = d_obst; a.X = d_X; a.U = d_U;
    a.winner = out->winner; a.best_key = out->best_key; a.best_u0 = out->best_u0; a.min_margin = out->min_margin;
    a.ep_flags = out->ep_flags; a.ep_steps = out->ep_steps; a.lost = out->lost; a.switched = out->switched;
    a.member_x = out->member_x; a.member_obst = out->member_obst; a.member_goal = out->member_goal; a.member_flags = out->member_flags;
    a.ip_rhit = p.ip_rhit; a.omask = p.omask;
    a.geom = guess_geom(h, p);
    hipLaunchKernelGGL(h->gg_mode ? mpc::group_step_kernel<true> : mpc::group_step_kernel<false>, dim3((groups + mpc::kGroupWaves - 1) / mpc::kGroupWaves),
                       dim3(mpc::kGroupThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_rollout_merit_dev(mpc_handle *h, int batch, int members, const double *d_x0, const double *d_P, const double *d_goal, const double *d_X,
                          const double *d_U, double *d_merit, double *d_defect, double *d_margin, double *d_boxviol, double *d_Xr, void *stream)
{
    // (what needs no handle is judged first: the same answers with and without a device)
    if (batch < 1) return fail(MPC_ERR_ARG, "batch outside [1, max_batch]");
    if (members < 1) return fail(MPC_ERR_ARG, "members must be >= 1");
    if (!d_merit && !d_defect && !d_margin && !d_boxviol && !d_Xr) return fail(MPC_ERR_ARG, "no output asked for");
    if (d_defect && !d_X) return fail(MPC_ERR_ARG, "d_defect needs d_X (the defect is that of a given iterate)");
    if (!d_x0 || !d_P || !d_goal || !d_U) return fail(MPC_ERR_ARG, "null device pointer (d_x0, d_P, d_goal and d_U are mandatory)");
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (batch > h->max_batch) return fail(MPC_ERR_ARG, "batch outside [1, max_batch]");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick(h, stream);
    // the constants and per-instance inputs of the solve that would be launched now: its kernel arguments, none of its outputs
    mpc::KParams p;
    int rc = beside_solve(h, batch, d_x0, d_P, d_goal, s, true, p); if (rc) return rc;
    p.r_hit = 1.0 + 0.2;               // o.r + R_ROBOT, as mpc_closed_loop_step_dev sets it
    mpc::MeritArgs a = {d_U, d_X, d_merit, d_defect, d_margin, d_boxviol, d_Xr, members};
    hipLaunchKernelGGL(mpc::rollout_merit_kernel, dim3((batch + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, s, p, a);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_plant_step_dev(mpc_handle *h, int batch, const double *d_x, const double *d_u, double *d_xnext, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_x || !d_u || !d_xnext) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::plant_step_kernel, dim3((batch + 255) / 256), dim3(256), 0, pick(h, stream), batch, h->cfg.Tf / h->cfg.N, d_x, d_u, d_xnext);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_obstacle_step_dev(mpc_handle *h, int count, double *d_obst, const double *d_noise, double randomness, double vmax, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (count < 0 || count > h->max_batch * h->cfg.n_obst) return fail(MPC_ERR_ARG, "count outside [0, max_batch * n_obst]");
    if (count == 0) return MPC_OK;
    if (!d_obst) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::obstacle_step_kernel, dim3((count + 255) / 256), dim3(256), 0, pick(h, stream), make_world(h->cfg), count,
                       h->cfg.Tf / h->cfg.N, d_obst, d_noise, randomness, vmax);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_generate_scenarios_dev(mpc_handle *h, int count, int scenario, unsigned seed0, const double *box, double *d_obst, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (count < 0 || count > h->max_batch) return fail(MPC_ERR_ARG, "count outside [0, max_batch]");
    if (scenario < 0 || scenario > 2) return fail(MPC_ERR_ARG, "scenario must be 0 (RANDOM), 1 (CENTER) or 2 (EDGE)");
    if (count == 0) return MPC_OK;
    if (!box || !d_obst) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    if (wide_rows(h->cfg.n_obst))      // (more draws than the first regeneration of the generator's state covers from the seeded words)
        hipLaunchKernelGGL(mpc::scenario_wide_kernel, dim3((count + 63) / 64), dim3(64), 0, pick(h, stream), count, h->cfg.n_obst, scenario, seed0,
                           box[0], box[1], box[2], box[3], box[4], box[5], d_obst);
    else
        hipLaunchKernelGGL(mpc::scenario_kernel, dim3((count + 63) / 64), dim3(64), 0, pick(h, stream), count, h->cfg.n_obst, scenario, seed0,
                           box[0], box[1], box[2], box[3], box[4], box[5], d_obst);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_linearize_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_P, const double *d_goal,
                      const double *d_X, const double *d_U, double *d_A, double *d_B, double *d_b, double *d_q,
                      double *d_hval, double *d_dh, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_x0 || !d_P || !d_goal || !d_X || !d_U || !d_A || !d_B || !d_b || !d_q || !d_hval || !d_dh) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    mpc::KParams p = make_params(h->cfg, batch);
    p.x0 = d_x0; p.P = d_P; p.goal = d_goal;
    const int count = batch * (h->cfg.N + 1);
    rc = attach_inputs(h, p, pick(h, stream), kForLinearize); if (rc) return rc;
    if (p.ip_w)
        hipLaunchKernelGGL((mpc::linearize_kernel<true, true>), dim3((count + 127) / 128), dim3(128), 0, pick(h, stream), p, h->cfg.n_obst, d_X, d_U,
                           d_A, d_B, d_b, d_q, d_hval, d_dh);
    else if (h->d_yref)
        hipLaunchKernelGGL(mpc::linearize_kernel<true>, dim3((count + 127) / 128), dim3(128), 0, pick(h, stream), p, h->cfg.n_obst, d_X, d_U,
                           d_A, d_B, d_b, d_q, d_hval, d_dh);
    else
        hipLaunchKernelGGL(mpc::linearize_kernel<false>, dim3((count + 127) / 128), dim3(128), 0, pick(h, stream), p, h->cfg.n_obst, d_X, d_U,
                           d_A, d_B, d_b, d_q, d_hval, d_dh);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_debug_adjoint_dev(mpc_handle *h, int batch, int lanes_per_instance, int lanes_per_stage, const double *d_X, const double *d_U, const double *d_g,
                          double *d_ru, void *stream)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!d_X || !d_U || !d_g || !d_ru) return fail(MPC_ERR_ARG, "null device pointer");
    const int N = h->cfg.N, G = lanes_per_instance, L = lanes_per_stage;
    if (!(L == 1 || L == 2 || L == 3)) return fail(MPC_ERR_ARG, "lanes_per_stage must be 1, 2 or 3");
    if (L > 1 ? (L * (N + 1) > 64) : !((G == 16 || G == 21 || G == 32 || G == 64) && N + 1 <= G))
        return fail(MPC_ERR_ARG, "the horizon does not fit this lane layout");
    HIPCHK(hipSetDevice(h->device));
    mpc::KParams p = make_params(h->cfg, batch);
    hipStream_t s = pick(h, stream);
    const int ipw = L > 1 ? 1 : (G == 21 ? 3 : 64 / G);
    const dim3 grid((batch + ipw - 1) / ipw), block(64);
    if (L == 3) hipLaunchKernelGGL((mpc::adjoint_check_kernel<64, 3>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    else if (L == 2) hipLaunchKernelGGL((mpc::adjoint_check_kernel<64, 2>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    else if (G == 16) hipLaunchKernelGGL((mpc::adjoint_check_kernel<16, 1>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    else if (G == 21) hipLaunchKernelGGL((mpc::adjoint_check_kernel<21, 1>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    else if (G == 32) hipLaunchKernelGGL((mpc::adjoint_check_kernel<32, 1>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    else hipLaunchKernelGGL((mpc::adjoint_check_kernel<64, 1>), grid, block, 0, s, p, d_X, d_U, d_g, d_ru);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

/* ------------------------------------------------- host-pointer API ------------------------------------------------- */

int mpc_set_warmstart(mpc_handle *h, int batch, const double *X, const double *U)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (!X || !U) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    const size_t N = h->cfg.N;
    HIPCHK(hipMemcpyAsync(h->dX, X, (size_t)batch * (N + 1) * 5 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->dU, U, (size_t)batch * N * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_get_traj(mpc_handle *h, int batch, double *X, double *U)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t N = h->cfg.N;
    if (X) HIPCHK(hipMemcpyAsync(X, h->dX, (size_t)batch * (N + 1) * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (U) HIPCHK(hipMemcpyAsync(U, h->dU, (size_t)batch * N * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_reset_guess(mpc_handle *h, int batch, const double *x0)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (!x0) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_x0, x0, (size_t)batch * 5 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = mpc_reset_guess_dev(h, batch, h->d_x0, h->dX, h->dU, nullptr); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_reset_guess_interp(mpc_handle *h, int batch, const double *x0, const double *goal)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (!x0 || !goal) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_x0, x0, (size_t)batch * 5 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_goal, goal, (size_t)batch * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = mpc_reset_guess_interp_dev(h, batch, h->d_x0, h->d_goal, h->dX, h->dU, nullptr); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_shift(mpc_handle *h, int batch)
{
    int rc = mpc_shift_dev(h, batch, h ? h->dX : nullptr, h ? h->dU : nullptr, nullptr); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

static int solve_common(mpc_handle *h, int batch, const double *x0, const double *P, const double *obst, const double *goal,
                        double *u0, double *cost, int32_t *status, int32_t *iters)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!x0 || !goal || (!P && !obst)) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    const size_t N = h->cfg.N, no = h->cfg.n_obst;
    if (batch <= kPackBatch) {
        // The reference's own call pattern (one scenario, one solve per control step) is dominated by the eight small transfers and the
        // separate look-ahead launch of the general path below: here the inputs travel as ONE pinned block, the look-ahead is computed
        // inside the solve kernel (p.obst) and the four outputs come back as one block.
        const size_t B = (size_t)batch, nin = 7 * B + (P ? B * (N + 1) * no * 2 : B * no * 4);
        double *hin = h->h_pack, *hout = h->h_pack + (size_t)kPackBatch * h->pack_in;
        double *din = h->d_pack, *dout = h->d_pack + (size_t)kPackBatch * h->pack_in;
        memcpy(hin, x0, 5 * B * sizeof(double)); memcpy(hin + 5 * B, goal, 2 * B * sizeof(double));
        memcpy(hin + 7 * B, P ? P : obst, (nin - 7 * B) * sizeof(double));
        HIPCHK(hipMemcpyAsync(din, hin, nin * sizeof(double), hipMemcpyHostToDevice, h->stream));
        int32_t *dstat = (int32_t *)(dout + 3 * B);
        mpc::KParams p = solve_params(h, batch, din, P ? din + 7 * B : nullptr, P ? nullptr : din + 7 * B, din + 5 * B, h->dX, h->dU, dout, dout + 2 * B, dstat, dstat + B);
        rc = launch_solve(h, p, h->stream); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(hout, dout, 4 * B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (u0) memcpy(u0, hout, 2 * B * sizeof(double));
        if (cost) memcpy(cost, hout + 2 * B, B * sizeof(double));
        if (status) memcpy(status, hout + 3 * B, B * sizeof(int32_t));
        if (iters) memcpy(iters, (const int32_t *)(hout + 3 * B) + B, B * sizeof(int32_t));
        return MPC_OK;
    }
    HIPCHK(hipMemcpyAsync(h->d_x0, x0, (size_t)batch * 5 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_goal, goal, (size_t)batch * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (P) {
        HIPCHK(hipMemcpyAsync(h->d_P, P, (size_t)batch * (N + 1) * no * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        rc = mpc_solve_dev(h, batch, h->d_x0, h->d_P, h->d_goal, h->dX, h->dU, h->d_u0, h->d_cost, h->d_status, h->d_iters, nullptr);
    } else {        // obstacle states in: the look-ahead is computed inside the solve kernel (no P in HBM at all)
        HIPCHK(hipMemcpyAsync(h->d_obst, obst, (size_t)batch * no * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        mpc::KParams p = solve_params(h, batch, h->d_x0, nullptr, h->d_obst, h->d_goal, h->dX, h->dU, h->d_u0, h->d_cost, h->d_status, h->d_iters);
        rc = launch_solve(h, p, h->stream);
    }
    if (rc) return rc;
    if (u0) HIPCHK(hipMemcpyAsync(u0, h->d_u0, (size_t)batch * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (cost) HIPCHK(hipMemcpyAsync(cost, h->d_cost, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, h->d_status, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (iters) HIPCHK(hipMemcpyAsync(iters, h->d_iters, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_solve(mpc_handle *h, int batch, const double *x0, const double *P, const double *goal,
              double *u0, double *cost, int32_t *status, int32_t *iters)
{
    if (!P) return fail(MPC_ERR_ARG, "null pointer");
    return solve_common(h, batch, x0, P, nullptr, goal, u0, cost, status, iters);
}

int mpc_solve_obst(mpc_handle *h, int batch, const double *x0, const double *obst, const double *goal,
                   double *u0, double *cost, int32_t *status, int32_t *iters)
{
    if (!obst) return fail(MPC_ERR_ARG, "null pointer");
    return solve_common(h, batch, x0, nullptr, obst, goal, u0, cost, status, iters);
}

int mpc_plant_step(mpc_handle *h, int batch, const double *x, const double *u, double *x_next)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!x || !u || !x_next) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_xa, x, (size_t)batch * 5 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ua, u, (size_t)batch * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = mpc_plant_step_dev(h, batch, h->d_xa, h->d_ua, h->d_xb, nullptr); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(x_next, h->d_xb, (size_t)batch * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_predict(mpc_handle *h, int batch, const double *obst, double *P)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (batch == 0) return MPC_OK;
    if (!obst || !P) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    const size_t N = h->cfg.N, no = h->cfg.n_obst;
    HIPCHK(hipMemcpyAsync(h->d_obst, obst, (size_t)batch * no * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = mpc_predict_dev(h, batch, h->d_obst, h->d_P, nullptr); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(P, h->d_P, (size_t)batch * (N + 1) * no * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

int mpc_generate_scenarios(mpc_handle *h, int count, int scenario, unsigned seed0, const double *box, double *obst)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (count == 0) return MPC_OK;
    if (!obst) return fail(MPC_ERR_ARG, "null pointer");
    int rc = mpc_generate_scenarios_dev(h, count, scenario, seed0, box, h->d_obst, nullptr); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(obst, h->d_obst, (size_t)count * h->cfg.n_obst * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

/* ------------------------------------------------- the reference's noise stream -------------------------------------------------- */

int mpc_noise_state_words(void) { return mpc::kNoiseStateWords; }

int mpc_noise_init_dev(mpc_handle *h, int count, int scenario, unsigned seed0, uint32_t *d_state, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (count < 0 || scenario < 0 || scenario > 2) return fail(MPC_ERR_ARG, "bad count or scenario");
    if (count == 0) return MPC_OK;
    if (!d_state) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::noise_init_kernel, dim3((count + 63) / 64), dim3(64), 0, pick(h, stream), count, h->cfg.n_obst, scenario, seed0, d_state);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_noise_draw_dev(mpc_handle *h, int count, uint32_t *d_state, double *d_noise, const int32_t *d_ep_flags, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (count < 0) return fail(MPC_ERR_ARG, "bad count");
    if (count == 0) return MPC_OK;
    if (!d_state || !d_noise) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::noise_draw_kernel, dim3((count + 63) / 64), dim3(64), 0, pick(h, stream), count, h->cfg.n_obst, d_state, d_noise, d_ep_flags);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

/* ------------------------------------------------- seed sweeps: on-device episode refill -------------------------------------------------- */

int mpc_episode_refill_dev(mpc_handle *h, int slots, int scenario, unsigned seed_first, int seed_count, int max_steps, int flags, const double *box,
                           const double *d_start, const double *d_goal_rows, int per_seed, double *d_x0, double *d_obst, double *d_goal, double *d_X,
                           double *d_U, double *d_min_margin, int32_t *d_ep_flags, int32_t *d_ep_steps, uint32_t *d_state, double *d_noise,
                           int32_t *d_slot_seed, int32_t *d_cursor, double *d_res_f, int32_t *d_res_i, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (slots < 1 || slots > h->max_batch) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: slots outside [1, max_batch]");
    if (scenario < 0 || scenario > 2) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: scenario must be 0 (RANDOM), 1 (CENTER) or 2 (EDGE)");
    if (seed_count < 0) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: seed_count must be >= 0");
    if (max_steps < 1) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: max_steps must be >= 1");
    if (flags & ~(MPC_REFILL_ALIAS_BUG | MPC_REFILL_INTERP_GUESS | MPC_REFILL_DRAW_NOISE)) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: unknown flag");
    if (per_seed != 0 && per_seed != 1) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: per_seed must be 0 or 1");
    if (!box || !d_start || !d_goal_rows) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: null box, start or goal rows");
    if (!d_x0 || !d_obst || !d_goal || !d_X || !d_U || !d_min_margin || !d_ep_flags || !d_ep_steps || !d_state)
        return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: null slot array");
    if ((flags & MPC_REFILL_DRAW_NOISE) && !d_noise) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: MPC_REFILL_DRAW_NOISE without a noise array");
    if (!d_slot_seed || !d_cursor) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: null slot_seed or cursor");
    if (!d_res_f || !d_res_i) return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: null result array");
    if (h->ring_cap && h->ring_filled && (scenario != h->ring_scenario || seed_first != h->ring_seed_first || seed_count != h->ring_seed_count ||
                                          memcmp(box, h->ring_box, sizeof(h->ring_box)) != 0))
        return fail(MPC_ERR_ARG, "mpc_episode_refill_dev: scenario, seed_first, seed_count or box differ from those of the ring's last fill (mpc_episode_ring_fill_dev)");
    HIPCHK(hipSetDevice(h->device));
    int rc = own(h, &h->d_refill_assign, (size_t)h->max_batch); if (rc) return rc;
    hipStream_t s = pick(h, stream);
    hipLaunchKernelGGL(mpc::refill_decide_kernel, dim3(1), dim3(mpc::kRefillThreads), 0, s, slots, seed_count, max_steps, d_ep_flags, d_ep_steps,
                       h->d_refill_assign, d_cursor);
    if (!h->rt_on && !h->ring_cap) {      // a handle on which neither was set launches what it always has
        hipLaunchKernelGGL(mpc::refill_apply_kernel, dim3((slots + 63) / 64), dim3(64), 0, s, slots, h->cfg.n_obst, h->cfg.N, scenario, seed_first, flags, per_seed,
                           box[0], box[1], box[2], box[3], box[4], box[5], h->d_refill_assign, d_start, d_goal_rows, d_x0, d_obst, d_goal, d_X, d_U,
                           d_min_margin, d_ep_flags, d_ep_steps, d_state, d_noise, d_slot_seed, d_res_f, d_res_i);
    } else {
        mpc::RefillExtra ex;
        memset(&ex, 0, sizeof(ex));
        if (h->rt_on) {
            const mpc_refill_tables &t = h->rt;
            ex.W = t.W; ex.We = t.We; ex.r_safe = t.r_safe; ex.r_hit = t.r_hit; ex.mask = t.mask; ex.bounds = t.bounds;
            ex.slot_W = t.slot_W; ex.slot_We = t.slot_We; ex.slot_r_safe = t.slot_r_safe; ex.slot_r_hit = t.slot_r_hit; ex.slot_mask = t.slot_mask; ex.slot_bounds = t.slot_bounds;
            ex.log = t.log; ex.res_log = t.res_log;
        }
        ex.ring_cap = h->ring_cap; ex.ring_state = h->ring_state; ex.ring_obst = h->ring_obst; ex.ring_tag = h->ring_tag; ex.seed_src = h->ring_seed_src;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((slots + 63) / 64), dim3(64), 0, s, slots, h->cfg.n_obst, h->cfg.N, scenario, seed_first, flags, per_seed,
                               box[0], box[1], box[2], box[3], box[4], box[5], (const int32_t *)h->d_refill_assign, d_start, d_goal_rows, d_x0, d_obst, d_goal, d_X, d_U,
                               d_min_margin, d_ep_flags, d_ep_steps, d_state, d_noise, d_slot_seed, d_res_f, d_res_i, ex);
        };
        if (h->rt_on && h->ring_cap) go(mpc::refill_apply_ext_kernel<true, true>);
        else if (h->rt_on) go(mpc::refill_apply_ext_kernel<true, false>);
        else go(mpc::refill_apply_ext_kernel<false, true>);
    }
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

static_assert(mpc::kGroupRefillMaxObst == MPC_MAX_OBST, "the kernel holds one group's scenario draws for the largest handle");
int mpc_group_refill_dev(mpc_handle *h, int groups, int K, int scenario, unsigned seed_first, int seed_count, int max_steps, const double *box,
                         const double *d_start, const double *d_goal_rows, int per_seed, const double *d_offsets, const mpc_group_refill_arrays *a,
                         void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (K < 1 || K > 64) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: K must be in [1, 64] (one member per lane of the group's wavefront)");
    if (groups < 1 || (long long)groups * K > h->max_batch) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: groups < 1 or groups * K > max_batch");
    if (scenario < 0 || scenario > 2) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: scenario must be 0 (RANDOM), 1 (CENTER) or 2 (EDGE)");
    if (seed_count < 0) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: seed_count must be >= 0");
    if (max_steps < 1) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: max_steps must be >= 1");
    if (per_seed != 0 && per_seed != 1) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: per_seed must be 0 or 1");
    if (!box || !d_start || !d_goal_rows || !d_offsets || !a) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: null box, start rows, goal rows, offsets or arrays");
    if (!a->x || !a->obst || !a->goal || !a->X || !a->U || !a->min_margin || !a->ep_flags || !a->ep_steps || !a->lost || !a->switched || !a->state)
        return fail(MPC_ERR_ARG, "mpc_group_refill_dev: null group array (x, obst, goal, X, U, min_margin, ep_flags, ep_steps, lost, switched, state)");
    if (!a->slot_seed || !a->cursor || !a->res_f || !a->res_i) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: null slot_seed, cursor or result array");
    if (!a->member_x || !a->member_obst || !a->member_goal || !a->member_flags) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: null member array");
    if (h->rt_on) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: per-seed tables and the status log (mpc_set_refill_tables_dev) are not offered for groups");
    if (h->ring_cap) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: the ring of seeded episodes (mpc_episode_ring_dev) is not offered for groups");
    if (h->trace_rows) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: per-seed trajectories (mpc_episode_trace_set_dev) are not offered for groups");
    if (h->grec_rows) return fail(MPC_ERR_ARG, "mpc_group_refill_dev: the per-group record (mpc_group_record_set_dev) is keyed by group, a sweep moves seeds between groups: not offered for groups that are refilled");
    HIPCHK(hipSetDevice(h->device));
    int rc = own(h, &h->d_refill_assign, (size_t)h->max_batch); if (rc) return rc;
    hipStream_t s = pick(h, stream);
    // the guess geometry reads the per-instance tables of the member solve (r_safe rows, obstacle mask), with that solve's coverage checks; off: none
    mpc::KParams p;
    rc = beside_solve(h, groups * K, nullptr, nullptr, nullptr, s, h->gg_mode != 0, p); if (rc) return rc;
    hipLaunchKernelGGL(mpc::refill_decide_kernel, dim3(1), dim3(mpc::kRefillThreads), 0, s, groups, seed_count, max_steps, a->ep_flags, a->ep_steps,
                       h->d_refill_assign, a->cursor);
    mpc::GroupRefillArgs ga;
    ga.geom = guess_geom(h, p);
    ga.groups = groups; ga.K = K; ga.N = h->cfg.N; ga.n_obst = h->cfg.n_obst; ga.scenario = scenario; ga.per_seed = per_seed; ga.seed_first = seed_first;
    ga.x_lo = box[0]; ga.x_hi = box[1]; ga.y_lo = box[2]; ga.y_hi = box[3]; ga.v_max = box[4]; ga.edge = box[5];
    ga.assign = h->d_refill_assign; ga.start = d_start; ga.goal_src = d_goal_rows; ga.offsets = d_offsets;
    ga.x = a->x; ga.obst = a->obst; ga.goal = a->goal; ga.X = a->X; ga.U = a->U; ga.min_margin = a->min_margin;
    ga.ep_flags = a->ep_flags; ga.ep_steps = a->ep_steps; ga.lost = a->lost; ga.switched = a->switched;
    ga.state = a->state; ga.slot_seed = a->slot_seed; ga.res_f = a->res_f; ga.res_i = a->res_i;
    ga.member_x = a->member_x; ga.member_obst = a->member_obst; ga.member_goal = a->member_goal; ga.member_flags = a->member_flags;
    hipLaunchKernelGGL(h->gg_mode ? mpc::group_refill_apply_kernel<true> : mpc::group_refill_apply_kernel<false>,
                       dim3((groups + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, s, ga);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_set_refill_tables_dev(mpc_handle *h, const mpc_refill_tables *t)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!t) { h->rt_on = false; memset(&h->rt, 0, sizeof(h->rt)); return MPC_OK; }
    const struct { const char *name; const void *src, *dst; } pairs[6] = {{"W", t->W, t->slot_W}, {"We", t->We, t->slot_We}, {"r_safe", t->r_safe, t->slot_r_safe},
                                                                          {"r_hit", t->r_hit, t->slot_r_hit}, {"mask", t->mask, t->slot_mask}, {"bounds", t->bounds, t->slot_bounds}};
    bool any = false;
    for (const auto &p : pairs) {
        if (p.src && !p.dst) return fail(MPC_ERR_ARG, "mpc_set_refill_tables_dev: %s is given without its per-slot destination slot_%s", p.name, p.name);
        any = any || p.src;
    }
    if ((t->log != nullptr) != (t->res_log != nullptr)) return fail(MPC_ERR_ARG, "mpc_set_refill_tables_dev: log and res_log come together (%s is null)", t->log ? "res_log" : "log");
    if (!any && !t->log) return fail(MPC_ERR_ARG, "mpc_set_refill_tables_dev: no source and no log given (NULL switches the tables off)");
    h->rt = *t; h->rt_on = true;
    return MPC_OK;
}

int mpc_episode_status_log_dev(mpc_handle *h, int slots, const int32_t *d_status, const int32_t *d_ep_flags, const int32_t *d_ep_steps, int32_t *d_log, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (slots < 1 || slots > h->max_batch) return fail(MPC_ERR_ARG, "mpc_episode_status_log_dev: slots outside [1, max_batch]");
    if (!d_status || !d_ep_flags || !d_ep_steps || !d_log) return fail(MPC_ERR_ARG, "mpc_episode_status_log_dev: null status, ep_flags, ep_steps or log");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::status_log_kernel, dim3((slots + 63) / 64), dim3(64), 0, pick(h, stream), slots, d_status, d_ep_flags, d_ep_steps, d_log);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

int mpc_episode_ring_dev(mpc_handle *h, int capacity, uint32_t *d_ring_state, double *d_ring_obst, int32_t *d_ring_tag, int32_t *d_seed_src)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (capacity < 0) return fail(MPC_ERR_ARG, "mpc_episode_ring_dev: capacity must be >= 0 (0 detaches the ring)");
    if (capacity > 0 && (!d_ring_state || !d_ring_obst || !d_ring_tag)) return fail(MPC_ERR_ARG, "mpc_episode_ring_dev: null ring_state, ring_obst or ring_tag");
    h->ring_filled = false;
    if (capacity == 0) { h->ring_cap = 0; h->ring_state = nullptr; h->ring_obst = nullptr; h->ring_tag = nullptr; h->ring_seed_src = nullptr; return MPC_OK; }
    h->ring_cap = capacity; h->ring_state = d_ring_state; h->ring_obst = d_ring_obst; h->ring_tag = d_ring_tag; h->ring_seed_src = d_seed_src;
    return MPC_OK;
}

int mpc_episode_ring_fill_dev(mpc_handle *h, int scenario, unsigned seed_first, int seed_count, const double *box, const int32_t *d_cursor, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->ring_cap) return fail(MPC_ERR_ARG, "mpc_episode_ring_fill_dev: no ring attached (mpc_episode_ring_dev)");
    if (scenario < 0 || scenario > 2) return fail(MPC_ERR_ARG, "mpc_episode_ring_fill_dev: scenario must be 0 (RANDOM), 1 (CENTER) or 2 (EDGE)");
    if (seed_count < 0) return fail(MPC_ERR_ARG, "mpc_episode_ring_fill_dev: seed_count must be >= 0");
    if (!box || !d_cursor) return fail(MPC_ERR_ARG, "mpc_episode_ring_fill_dev: null box or cursor");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc::ring_fill_kernel, dim3((h->ring_cap + 63) / 64), dim3(64), 0, pick(h, stream), h->ring_cap, h->cfg.n_obst, scenario, seed_first, seed_count,
                       box[0], box[1], box[2], box[3], box[4], box[5], d_cursor, h->ring_state, h->ring_obst, h->ring_tag);
    HIPCHK(hipGetLastError());
    h->ring_filled = true; h->ring_scenario = scenario; h->ring_seed_first = seed_first; h->ring_seed_count = seed_count;
    memcpy(h->ring_box, box, sizeof(h->ring_box));
    return MPC_OK;
}

int mpc_episode_trace_set_dev(mpc_handle *h, int rows, int max_steps, const mpc_episode_trace *t)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!t || rows == 0) { h->trace_rows = 0; h->trace_max_steps = 0; memset(&h->trace, 0, sizeof(h->trace)); return MPC_OK; }
    if (rows < 0) return fail(MPC_ERR_ARG, "mpc_episode_trace_set_dev: rows must be >= 0 (0 detaches the trace)");
    if (max_steps < 1) return fail(MPC_ERR_ARG, "mpc_episode_trace_set_dev: max_steps must be >= 1");
    const struct { const char *name; const void *p; } need[8] = {{"seed_row", t->seed_row}, {"slot_state", t->slot_state}, {"len", t->len}, {"x", t->x},
                                                                 {"obst", t->obst}, {"u", t->u}, {"status", t->status}, {"iters", t->iters}};
    for (const auto &f : need)
        if (!f.p) return fail(MPC_ERR_ARG, "mpc_episode_trace_set_dev: %s is null (pred alone may be)", f.name);
    h->trace = *t; h->trace_rows = rows; h->trace_max_steps = max_steps;
    return MPC_OK;
}

int mpc_episode_trace_dev(mpc_handle *h, int slots, int phase, const int32_t *d_slot_seed, const double *d_x0, const double *d_obst, const double *d_X,
                          const double *d_u0, const int32_t *d_status, const int32_t *d_iters, const int32_t *d_ep_flags, const int32_t *d_ep_steps, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->trace_rows) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: no trace attached (mpc_episode_trace_set_dev)");
    if (slots < 1 || slots > h->max_batch) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: slots outside [1, max_batch]");
    if (phase != MPC_TRACE_START && phase != MPC_TRACE_STEP) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: phase must be MPC_TRACE_START (0) or MPC_TRACE_STEP (1)");
    if (!d_slot_seed || !d_x0 || !d_obst || !d_ep_flags || !d_ep_steps) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: null slot_seed, x0, obst, ep_flags or ep_steps");
    if (phase == MPC_TRACE_STEP) {
        if (!d_u0) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: MPC_TRACE_STEP without u0 (hand the fused step a u0 array)");
        if (!d_status || !d_iters) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: MPC_TRACE_STEP without status or iters");
        if (h->trace.pred && !d_X) return fail(MPC_ERR_ARG, "mpc_episode_trace_dev: MPC_TRACE_STEP without X while the trace holds pred");
    }
    HIPCHK(hipSetDevice(h->device));
    const mpc_episode_trace &t = h->trace;
    mpc::TraceArrays a{t.seed_row, t.slot_state, t.len, t.x, t.obst, t.u, t.status, t.iters, t.pred, h->trace_rows, h->trace_max_steps};
    constexpr int per = mpc::kTraceThreads / 64;
    hipLaunchKernelGGL(mpc::episode_trace_kernel, dim3((slots + per - 1) / per), dim3(mpc::kTraceThreads), 0, pick(h, stream), slots, phase, h->cfg.n_obst, h->cfg.N,
                       a, d_slot_seed, d_x0, d_obst, d_X, d_u0, d_status, d_iters, d_ep_flags, d_ep_steps);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

/* ------------------------------------------------- multi-start episodes: the per-group record -------------------------------------------------- */

int mpc_group_record_set_dev(mpc_handle *h, int rows, int max_steps, int K, const mpc_group_record *r)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!r || rows == 0) { h->grec_rows = 0; h->grec_max_steps = 0; h->grec_K = 0; memset(&h->grec, 0, sizeof(h->grec)); return MPC_OK; }
    if (rows < 0) return fail(MPC_ERR_ARG, "mpc_group_record_set_dev: rows must be >= 0 (0 detaches the record)");
    if (max_steps < 1) return fail(MPC_ERR_ARG, "mpc_group_record_set_dev: max_steps must be >= 1");
    if (K < 1 || K > 64) return fail(MPC_ERR_ARG, "mpc_group_record_set_dev: K must be in [1, 64] (one member per lane of the group's wavefront)");
    const struct { const char *name; const void *p; } need[11] = {{"group_row", r->group_row}, {"len", r->len}, {"x", r->x}, {"obst", r->obst}, {"u", r->u},
                                                                  {"winner", r->winner}, {"best_key", r->best_key}, {"cand_key", r->cand_key},
                                                                  {"cand_status", r->cand_status}, {"cand_iters", r->cand_iters}, {"cand_u0", r->cand_u0}};
    for (const auto &f : need)
        if (!f.p) return fail(MPC_ERR_ARG, "mpc_group_record_set_dev: %s is null (cand_X alone may be)", f.name);
    h->grec = *r; h->grec_rows = rows; h->grec_max_steps = max_steps; h->grec_K = K;
    return MPC_OK;
}

int mpc_group_record_dev(mpc_handle *h, int groups, int K, int phase, const double *d_x, const double *d_obst, const double *d_X, const double *d_key,
                         const int32_t *d_status, const int32_t *d_iters, const double *d_u0, const mpc_group_step_out *out, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->grec_rows) return fail(MPC_ERR_ARG, "mpc_group_record_dev: no record attached (mpc_group_record_set_dev)");
    if (K < 1 || K > 64) return fail(MPC_ERR_ARG, "mpc_group_record_dev: K must be in [1, 64]");
    if (K != h->grec_K) return fail(MPC_ERR_ARG, "mpc_group_record_dev: K differs from the K the record was attached for (mpc_group_record_set_dev)");
    if (groups < 1 || (long long)groups * K > h->max_batch) return fail(MPC_ERR_ARG, "mpc_group_record_dev: groups < 1 or groups * K > max_batch");
    if (phase != MPC_GROUP_RECORD_SOLVED && phase != MPC_GROUP_RECORD_STEPPED)
        return fail(MPC_ERR_ARG, "mpc_group_record_dev: phase must be MPC_GROUP_RECORD_SOLVED (0) or MPC_GROUP_RECORD_STEPPED (1)");
    const struct { const char *name; const void *p; } need[8] = {{"d_x", d_x}, {"d_obst", d_obst}, {"d_X", d_X}, {"d_key", d_key}, {"d_status", d_status},
                                                                 {"d_iters", d_iters}, {"d_u0", d_u0}, {"out", out}};
    for (const auto &f : need)
        if (!f.p) return fail(MPC_ERR_ARG, "mpc_group_record_dev: %s is null", f.name);
    if (!out->winner || !out->ep_flags || !out->ep_steps) return fail(MPC_ERR_ARG, "mpc_group_record_dev: out->winner, out->ep_flags or out->ep_steps is null");
    if (phase == MPC_GROUP_RECORD_STEPPED && (!out->best_key || !out->best_u0))
        return fail(MPC_ERR_ARG, "mpc_group_record_dev: MPC_GROUP_RECORD_STEPPED without out->best_key or out->best_u0 (hand the group step both)");
    HIPCHK(hipSetDevice(h->device));
    const mpc_group_record &r = h->grec;
    mpc::GroupRecordArrays a{r.group_row, r.len, r.x, r.obst, r.u, r.winner, r.best_key, r.cand_key, r.cand_status, r.cand_iters, r.cand_u0, r.cand_X,
                             h->grec_rows, h->grec_max_steps};
    hipLaunchKernelGGL(mpc::group_record_kernel, dim3((groups + mpc::kGroupWaves - 1) / mpc::kGroupWaves), dim3(mpc::kGroupThreads), 0, pick(h, stream), groups, K, phase,
                       h->cfg.n_obst, h->cfg.N, a, d_x, d_obst, d_X, d_key, d_status, d_iters, d_u0, (const int32_t *)out->winner, (const double *)out->best_key,
                       (const double *)out->best_u0, (const int32_t *)out->ep_flags, (const int32_t *)out->ep_steps);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

/* ------------------------------------------------- multi-GPU: all-gather of the costs over RCCL -------------------------------------------------- */

namespace {
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
char g_rccl_err[256] = "";

int rccl_load()
{
    // handles on different threads may reach this together: one of them loads, the others wait (g_rccl is written once, before any reader returns)
    std::call_once(g_rccl_once, [] {
        void *lib = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { const char *e = dlerror(); snprintf(g_rccl_err, sizeof(g_rccl_err), "librccl.so.1 not found (%s): the cost exchange has no other transport", e ? e : "?"); return; }
        Rccl r; r.lib = lib;
        r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))dlsym(lib, "ncclCommInitRank");
        r.AllGather = (decltype(r.AllGather))dlsym(lib, "ncclAllGather");
        r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
        r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString) { dlclose(lib); snprintf(g_rccl_err, sizeof(g_rccl_err), "librccl lacks an entry point of the cost exchange"); return; }
        g_rccl = r;
    });
    if (!g_rccl.lib) return fail(MPC_ERR_HIP, "%s", g_rccl_err);
    return MPC_OK;
}
#define RCCLCHK(expr)                                                                                   \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) return fail(MPC_ERR_HIP, "%s: %s", #expr, g_rccl.GetErrorString(r_));    \
    } while (0)
}  // namespace

int mpc_comm_unique_id(unsigned char *id)
{
    static_assert(sizeof(ncclUniqueId) == MPC_COMM_ID_BYTES, "MPC_COMM_ID_BYTES is RCCL's ncclUniqueId");
    if (!id) return fail(MPC_ERR_ARG, "null id buffer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MPC_ERR_NODEVICE, "no HIP device visible: libmpcgpu has no CPU path");
    int rc = rccl_load(); if (rc) return rc;
    ncclUniqueId u;
    RCCLCHK(g_rccl.GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return MPC_OK;
}

int mpc_comm_init(mpc_handle *h, int rank, int world, const unsigned char *id)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(MPC_ERR_ARG, "bad rank / world / id");
    if (h->comm) return fail(MPC_ERR_ARG, "the handle has a communicator already (mpc_comm_destroy first)");
    int rc = rccl_load(); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    RCCLCHK(g_rccl.CommInitRank(&h->comm, world, u, rank));
    h->comm_rank = rank; h->comm_world = world;
    return MPC_OK;
}

int mpc_comm_world(const mpc_handle *h) { return h && h->comm ? h->comm_world : 0; }

int mpc_comm_library_path(char *buf, int len)
{
    if (!buf || len < 2) return fail(MPC_ERR_ARG, "bad buffer");
    int rc = rccl_load(); if (rc) return rc;
    Dl_info info;
    if (!dladdr((void *)g_rccl.AllGather, &info) || !info.dli_fname) return fail(MPC_ERR_HIP, "dladdr cannot name the library of ncclAllGather");
    snprintf(buf, (size_t)len, "%s", info.dli_fname);
    return MPC_OK;
}

int mpc_comm_destroy(mpc_handle *h)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->comm) return MPC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    RCCLCHK(g_rccl.CommDestroy(h->comm));       // on failure the handle keeps the communicator: the caller may retry, nothing leaks silently
    h->comm = nullptr; h->comm_world = 0; h->comm_rank = 0;
    (void)disown(h, h->d_gather_in); (void)disown(h, h->d_gather_out);      // sized for this communicator's world
    h->gather_cap = 0;
    return MPC_OK;
}

int mpc_allgather_cost_dev(mpc_handle *h, int count, const double *d_cost, double *d_cost_all, void *stream)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->comm) return fail(MPC_ERR_ARG, "no communicator: mpc_comm_init first");
    if (count < 0) return fail(MPC_ERR_ARG, "bad count");
    if (count == 0) return MPC_OK;
    if (!d_cost || !d_cost_all) return fail(MPC_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(h->device));
    RCCLCHK(g_rccl.AllGather(d_cost, d_cost_all, (size_t)count, ncclDouble, h->comm, pick(h, stream)));
    return MPC_OK;
}

int mpc_allgather_cost(mpc_handle *h, int count, const double *cost, double *cost_all)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!h->comm) return fail(MPC_ERR_ARG, "no communicator: mpc_comm_init first");
    if (count < 0) return fail(MPC_ERR_ARG, "bad count");
    if (count == 0) return MPC_OK;
    if (!cost || !cost_all) return fail(MPC_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(h->device));
    if ((size_t)count > h->gather_cap) {
        (void)disown(h, h->d_gather_in); (void)disown(h, h->d_gather_out);
        h->gather_cap = 0;
        int rc = own(h, &h->d_gather_in, (size_t)count);
        if (!rc) rc = own(h, &h->d_gather_out, (size_t)count * h->comm_world);
        if (rc) return rc;
        h->gather_cap = (size_t)count;
    }
    HIPCHK(hipMemcpyAsync(h->d_gather_in, cost, (size_t)count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = mpc_allgather_cost_dev(h, count, h->d_gather_in, h->d_gather_out, nullptr); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(cost_all, h->d_gather_out, (size_t)count * h->comm_world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPC_OK;
}

/* ------------------------------------------------- slack schedule -------------------------------------------------- */

static int slack_schedule_off(mpc_handle *h) { h->alpha = {}; h->d_alpha = nullptr; return MPC_OK; }

int mpc_set_slack_schedule_dev(mpc_handle *h, const double *d_alpha)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!d_alpha) return slack_schedule_off(h);
    h->d_alpha = d_alpha; h->alpha = {2, h->max_batch};
    return MPC_OK;
}

int mpc_set_slack_schedule(mpc_handle *h, int batch, const double *alpha)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (!alpha) return slack_schedule_off(h);
    if (batch == 0) return fail(MPC_ERR_ARG, "a slack schedule needs batch >= 1");
    HIPCHK(hipSetDevice(h->device));
    const size_t row = (size_t)h->cfg.N + 1;
    for (size_t k = 0; k < (size_t)batch * row; k++)
        if (!(alpha[k] >= 0.0) || !(alpha[k] <= 1e300)) return fail(MPC_ERR_ARG, "slack weights must be finite and >= 0");
    rc = upload(h, &h->d_alpha_own, (size_t)h->max_batch * row, alpha, (size_t)batch * row); if (rc) return rc;
    h->d_alpha = h->d_alpha_own; h->alpha = {1, batch};
    return MPC_OK;
}

/* ------------------------------------------------ per-stage reference ------------------------------------------------ */

static int reference_off(mpc_handle *h) { h->ref = {}; h->d_yref = nullptr; h->d_ref_off = nullptr; h->ref_T = 0; return MPC_OK; }

int mpc_set_reference(mpc_handle *h, int batch, int T, const double *yref, const int32_t *offset)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!yref) return reference_off(h);
    if (batch < 1 || batch > h->max_batch) return fail(MPC_ERR_ARG, "a per-stage reference needs batch in [1, max_batch]");
    if (T < 1) return fail(MPC_ERR_ARG, "a per-stage reference needs T >= 1 rows");
    const size_t n = (size_t)batch * T * 6;
    for (size_t k = 0; k < n; k++)
        if (!(yref[k] >= -1e300 && yref[k] <= 1e300)) return fail(MPC_ERR_ARG, "reference entries must be finite");
    if (offset)
        for (int b = 0; b < batch; b++)
            if (offset[b] < 0) return fail(MPC_ERR_ARG, "reference offsets must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    const size_t cap = (size_t)h->max_batch * T * 6;
    if (h->yref_own_cap < cap) {      // the copy grows: the one place that switches a feature off before the call can still fail
        HIPCHK(hipStreamSynchronize(h->stream));      // (an earlier solve may still read the old copy)
        reference_off(h); h->yref_own_cap = 0;
        int rc = disown(h, h->d_yref_own); if (rc) return rc;
        rc = own(h, &h->d_yref_own, cap); if (rc) return rc;
        h->yref_own_cap = cap;
    }
    int rc = upload(h, &h->d_yref_own, cap, yref, n);
    if (!rc && offset) rc = upload(h, &h->d_ref_off_own, (size_t)h->max_batch, offset, (size_t)batch);
    if (rc) return rc;
    h->d_yref = h->d_yref_own; h->d_ref_off = offset ? h->d_ref_off_own : nullptr;
    h->ref_T = T; h->ref = {1, batch};
    return MPC_OK;
}

int mpc_set_reference_dev(mpc_handle *h, int T, const double *d_yref, int32_t *d_offset)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!d_yref) return reference_off(h);
    if (T < 1) return fail(MPC_ERR_ARG, "a per-stage reference needs T >= 1 rows");
    h->d_yref = d_yref; h->d_ref_off = d_offset;
    h->ref_T = T; h->ref = {2, h->max_batch};
    return MPC_OK;
}

/* ---------------------------------------------- per-instance parameters ---------------------------------------------- */

static int instance_params_off(mpc_handle *h) { h->ip = {}; return MPC_OK; }

int mpc_set_instance_params(mpc_handle *h, int batch, const double *W, const double *We, const double *r_safe, const double *r_hit)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!W && !We && !r_safe && !r_hit) return instance_params_off(h);
    if (batch < 1 || batch > h->max_batch) return fail(MPC_ERR_ARG, "per-instance parameters need batch in [1, max_batch]");
    const size_t B = (size_t)batch, no = (size_t)h->cfg.n_obst;
    auto all_in = [](const double *v, size_t n, double lo, bool open) {      // finite and >= lo (open: > lo); NaN fails every comparison
        if (!v) return true;
        for (size_t k = 0; k < n; k++)
            if (!((open ? v[k] > lo : v[k] >= lo) && v[k] <= 1e300)) return false;
        return true;
    };
    if (!all_in(W, B * 6, 0.0, false) || !all_in(We, B * 4, 0.0, false)) return fail(MPC_ERR_ARG, "per-instance weights must be finite and >= 0");
    if (!all_in(r_safe, B * no, 0.0, true) || !all_in(r_hit, B * no, 0.0, true)) return fail(MPC_ERR_ARG, "per-instance radii must be finite and > 0");
    HIPCHK(hipSetDevice(h->device));
    int rc = upload_instance_tables(h, h->ip_own, batch, W, We, r_safe, r_hit); if (rc) return rc;
    h->ip = {1, batch};
    return MPC_OK;
}

int mpc_set_instance_params_dev(mpc_handle *h, const double *d_W, const double *d_We, const double *d_r_safe, const double *d_r_hit)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!d_W && !d_We && !d_r_safe && !d_r_hit) return instance_params_off(h);
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->max_batch, no = (size_t)h->cfg.n_obst;      // the tables attach_inputs derives into, in front of every solve
    int rc = own(h, &h->ip_own.w, B * mpc::kIpW);
    if (!rc) rc = own(h, &h->ip_own.r2, B * no);
    if (!rc) rc = own(h, &h->ip_own.rhit, B * no);
    if (rc) return rc;
    h->ip_dev[0] = d_W; h->ip_dev[1] = d_We; h->ip_dev[2] = d_r_safe; h->ip_dev[3] = d_r_hit;
    h->ip = {2, h->max_batch};
    return MPC_OK;
}

/* ---------------------------------------------- per-instance obstacle masks ---------------------------------------------- */

static int obstacle_mask_off(mpc_handle *h) { h->om = {}; h->d_omask = nullptr; return MPC_OK; }

int mpc_set_obstacle_mask(mpc_handle *h, int batch, const uint32_t *mask)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!mask) return obstacle_mask_off(h);
    if (batch < 1 || batch > h->max_batch) return fail(MPC_ERR_ARG, "an obstacle mask needs batch in [1, max_batch]");
    for (int b = 0; b < batch; b++)
        if (mask[b] & ~all_obstacles(h)) return fail(MPC_ERR_ARG, "an obstacle mask word has a bit at or above n_obst");
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_companions(h, 3);
    if (!rc) rc = upload(h, &h->d_omask_own, (size_t)h->max_batch, mask, (size_t)batch);
    if (rc) return rc;
    h->d_omask = h->d_omask_own; h->om = {1, batch};
    return MPC_OK;
}

int mpc_set_obstacle_mask_dev(mpc_handle *h, const uint32_t *d_mask)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!d_mask) return obstacle_mask_off(h);
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_companions(h, 3); if (rc) return rc;
    h->d_omask = d_mask; h->om = {2, h->max_batch};
    return MPC_OK;
}

/* ---------------------------------------------- per-instance box bounds ---------------------------------------------- */

static int instance_bounds_off(mpc_handle *h) { h->bd = {}; h->d_ip_b = nullptr; return MPC_OK; }

int mpc_set_instance_bounds(mpc_handle *h, int batch, const double *bx_lo, const double *bx_hi, const double *bu_lo, const double *bu_hi)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!bx_lo && !bx_hi && !bu_lo && !bu_hi) return instance_bounds_off(h);
    if (batch < 1 || batch > h->max_batch) return fail(MPC_ERR_ARG, "instance bounds need batch in [1, max_batch]");
    std::vector<double> tab;
    int rc = pack_bounds(h, batch, bx_lo, bx_hi, bu_lo, bu_hi, tab); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_companions(h, 4);
    if (!rc) rc = upload(h, &h->d_ip_b_own, tab.size(), tab.data(), tab.size());
    if (rc) return rc;
    h->d_ip_b = h->d_ip_b_own; h->bd = {1, batch};
    return MPC_OK;
}

int mpc_set_instance_bounds_dev(mpc_handle *h, const double *d_bounds)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (!d_bounds) return instance_bounds_off(h);
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_companions(h, 4); if (rc) return rc;
    h->d_ip_b = d_bounds; h->bd = {2, h->max_batch};
    return MPC_OK;
}

/* ---------------------------------------------- several SQP iterations per launch ---------------------------------------------- */

int mpc_set_sqp(mpc_handle *h, int max_iter, double step_tol)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (max_iter < 1 || max_iter > MPC_MAX_SQP_ITER) return fail(MPC_ERR_ARG, "mpc_set_sqp: max_iter must be in [1, MPC_MAX_SQP_ITER]");
    if (!(step_tol >= 0.0)) return fail(MPC_ERR_ARG, "mpc_set_sqp: step_tol must be >= 0 (+inf is valid, NaN is not)");
    if (max_iter > 1) {
        HIPCHK(hipSetDevice(h->device));
        int rc = ensure_companions(h, 5); if (rc) return rc;
    }
    h->sqp_max = max_iter; h->sqp_tol = step_tol;
    return MPC_OK;
}

int mpc_set_sqp_iters_out_dev(mpc_handle *h, int32_t *d_sqp_iters)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->d_sqp_iters = d_sqp_iters;
    return MPC_OK;
}

/* --------------------------------------------------- measurement --------------------------------------------------- */

int mpc_profile_enable(mpc_handle *h, int on)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->profiling = on > 0 ? on : 0;
    h->ev_used = 0; h->launch_count = 0;
    if (on) {   // event pool up front, so that no event is created inside a timed region
        HIPCHK(hipSetDevice(h->device));
        while ((int)h->ev_start.size() < kMaxEvents) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
            h->ev_start.push_back(a); h->ev_stop.push_back(b);
        }
    }
    return MPC_OK;
}

int mpc_profile_read(mpc_handle *h, double *sum_ms, int *launches)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    double sum = 0.0;
    for (int k = 0; k < h->ev_used; k++) {
        HIPCHK(hipEventSynchronize(h->ev_stop[k]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_start[k], h->ev_stop[k]));
        sum += ms;
    }
    if (sum_ms) *sum_ms = sum;
    if (launches) *launches = h->ev_used;
    h->ev_used = 0;
    return MPC_OK;
}

int mpc_set_accumulators(mpc_handle *h, int32_t *d_iters_acc, int32_t *d_status_acc)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->d_iters_acc = d_iters_acc; h->d_status_acc = d_status_acc;
    return MPC_OK;
}

int mpc_debug_trace(mpc_handle *h, int enable, int batch, double *host_out)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (host_out && (batch < 1 || batch > h->max_batch)) return fail(MPC_ERR_ARG, "mpc_debug_trace: batch outside [1, max_batch]");
    HIPCHK(hipSetDevice(h->device));
    const size_t count = (size_t)h->max_batch * h->cfg.qp_iter_max * 4;
    if (enable && !h->d_trace) { int rc = own(h, &h->d_trace, count); if (rc) return rc; HIPCHK(hipMemset(h->d_trace, 0, count * sizeof(double))); }
    if (host_out && h->d_trace) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(host_out, h->d_trace, (size_t)batch * h->cfg.qp_iter_max * 4 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return enable ? MPC_OK : disown(h, h->d_trace);
}

int mpc_set_lanes_per_instance(mpc_handle *h, int lanes)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (lanes != 0 && lanes != 16 && lanes != 21 && lanes != 32 && lanes != 64) return fail(MPC_ERR_ARG, "lanes must be 0 (automatic), 16, 21, 32 or 64");
    if (lanes == 21 ? h->cfg.N > 20 : (lanes != 0 && lanes < h->cfg.N + 2)) return fail(MPC_ERR_ARG, "lanes per instance must exceed N + 1 (21 lanes: N <= 20)");
    h->lanes_override = lanes;
    return MPC_OK;
}

int mpc_set_matrix_cores(mpc_handle *h, int on)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->use_mfma = on ? 1 : 0;
    return MPC_OK;
}

int mpc_set_row_parallel(mpc_handle *h, int on)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->row_parallel = on ? 1 : 0;
    return MPC_OK;
}

int mpc_set_block_riccati(mpc_handle *h, int on)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->block2 = on ? 1 : 0;
    return MPC_OK;
}

int mpc_get_lanes_per_instance(mpc_handle *h, int batch)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    return pick_split(h, batch) > 1 ? 64 : pick_lanes(h, batch);
}

int mpc_set_lanes_per_stage(mpc_handle *h, int lanes)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (lanes < 0 || lanes > 3) return fail(MPC_ERR_ARG, "lanes per stage must be 0 (automatic), 1, 2 or 3");
    if ((lanes == 3 && h->cfg.N > 20) || (lanes == 2 && h->cfg.N > 31)) return fail(MPC_ERR_ARG, "lanes per stage * (N + 1) must not exceed 64");
    h->split_override = lanes;
    return MPC_OK;
}

int mpc_get_lanes_per_stage(mpc_handle *h, int batch)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    return pick_split(h, batch);
}

int mpc_set_instance_scheduling(mpc_handle *h, int on)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    h->scheduling = on ? 1 : 0;
    h->order_batch = 0;
    return MPC_OK;
}

int mpc_get_instance_order(mpc_handle *h, int batch, int32_t *order)
{
    int rc = check_batch(h, batch); if (rc) return rc;
    if (!order) return fail(MPC_ERR_ARG, "null pointer");
    if (h->order_batch != batch) return 0;          // no order in effect for this batch size: natural order
    HIPCHK(hipSetDevice(h->device));
    if (h->sched_done) HIPCHK(hipEventSynchronize(h->sched_done));      // the order was built on the stream of the launch that preceded it, not necessarily ours
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(order, h->d_order, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 1;
}

int mpc_get_kernel_name(mpc_handle *h, int batch, int lookahead, char *buf, int len)
{
    if (!h || !buf || len < 1) return fail(MPC_ERR_ARG, "null argument");
    const mpc::SolvePlan q = plan_solve(h, batch, lookahead != 0);
    const int rc = check_plan(h, q); if (rc) return rc;
    mpc::format_kernel_name(q, buf, (size_t)len);      // (a name also where the table has no such row: the launch then refuses)
    return MPC_OK;
}

int mpc_set_waves_per_simd(mpc_handle *h, int waves)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    if (waves < 0 || waves > 2) return fail(MPC_ERR_ARG, "wavefronts per SIMD must be 0 (automatic), 1 or 2");
    h->waves_override = waves;
    return MPC_OK;
}

int mpc_get_waves_per_simd(mpc_handle *h, int batch)
{
    if (!h) return fail(MPC_ERR_ARG, "null handle");
    return pick_split(h, batch) > 1 ? pick_waves(h, batch) : 1;
}

}  // extern "C"
