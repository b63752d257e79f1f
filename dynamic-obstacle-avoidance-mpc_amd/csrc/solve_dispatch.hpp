// solve_dispatch.hpp -- the solve kernels libmpcgpu.so is built with, as ONE table, and the plan that names one of them.
// A row of kSolveKernels is the only place its instantiation is mentioned: the table is the list of device instantiations (what decides compile
// time and what the ISA audit reads).  A launch is plan_solve (mpc_api.hip) -> find_solve_kernel -> launch through the row's function pointer;
// mpc_get_kernel_name formats the same plan.
#pragma once
#include "rti_kernel.hpp"
#include "rti_split_kernel.hpp"
#include "rti_wide_kernel.hpp"

#include <stdint.h>
#include <stdio.h>

namespace mpc {

enum Family { kOneLane = 0, kSplit = 1, kWide = 2 };      // rti_solve_kernel, rti_split_kernel, rti_wide_kernel

// the template arguments of an instantiation in one word.  a, b, c are the family's shape arguments: (G, FACT, -) one lane per stage,
// (LPS, W2, BLK2) stage-split, (LPS, -, -) multi-wavefront; level: 0 none, 1 REF, 2 REF + IPAR, 3 REF + IPAR + OSEL, 4 REF + IPAR + OSEL + IBND, 5 REF + IPAR + OSEL + IBND + NSQP (the kernels' static_asserts nest them so)
constexpr uint32_t solve_key(int family, int cap, int a, int b, int c, bool masked, int level)
{
    if (family > 3 || cap > 63 || a > 127 || b > 3 || c > 1 || level > 7) throw "solve_key: a field does not fit";      // (in the table: a compile error)
    return (uint32_t)family | (uint32_t)cap << 2 | (uint32_t)a << 8 | (uint32_t)b << 15 | (uint32_t)c << 17 | (uint32_t)masked << 18 | (uint32_t)level << 19;
}

struct KernelRow {
    uint32_t key;
    int block;                                   // threads per workgroup
    void (*fn)(const KParams);
    size_t (*lds)(int N, bool lookahead);        // dynamic LDS in bytes
};

// Dynamic LDS of rti_solve_kernel<no, G, fact>.  Compact stage blocks (fact 3; with ten row pairs the look-ahead positions stay resident behind the
// blocks, rti_kernel.hpp PLDS); otherwise the look-ahead positions, the matrix-core workspace (fact 1) and the dense row-parallel blocks (fact 2)
constexpr size_t one_lane_lds(int no, int G, int fact, int N, bool lookahead)
{
    const int ipw = 64 / G;
    if (fact == 3) return (size_t)(no >= 10 ? RowLdsC::total_with_positions(N, ipw, no) : RowLdsC::total(N, ipw)) * sizeof(double);
    return ((lookahead ? (size_t)ipw * (N + 1) * no * 2 : 0) + (fact == 1 ? (size_t)MfmaLds::doubles(N) : 0) + (fact == 2 ? (size_t)RowLds::total(N, ipw) : 0)) * sizeof(double);
}

template <int NO, int G, int FACT, bool MASKED, int L>
constexpr KernelRow one_lane()
{
    return {solve_key(kOneLane, NO, G, FACT, 0, MASKED, L), 64, &rti_solve_kernel<NO, G, FACT, MASKED, (L >= 1), (L >= 2), (L >= 3), (L >= 4), (L >= 5)>,
            [](int N, bool lookahead) { return one_lane_lds(NO, G, FACT, N, lookahead); }};
}

template <int NO, int LPS, bool W2, bool MASKED, bool BLK2, int L>
constexpr KernelRow split()
{
    return {solve_key(kSplit, NO, LPS, W2, BLK2, MASKED, L), 64, &rti_split_kernel<NO, LPS, W2, MASKED, BLK2, (L >= 1), (L >= 2), (L >= 3), (L >= 4), (L >= 5)>,
            [](int N, bool lookahead) { return (size_t)SplitLds<LPS, NO, W2, BLK2>::total(N, lookahead) * sizeof(double); }};
}

// 11 .. 32 obstacles: one instance per workgroup of WideShape<CAP>::W wavefronts
template <int CAP, bool MASKED, int L>
constexpr KernelRow wide()
{
    return {solve_key(kWide, CAP, 2, 0, 0, MASKED, L), 64 * WideShape<CAP>::W, &rti_wide_kernel<CAP, 2, MASKED, (L >= 1), (L >= 2), (L >= 3), (L >= 4), (L >= 5)>,
            [](int N, bool lookahead) { return (size_t)WideLds<CAP>::total(N, lookahead) * sizeof(double); }};
}

// The plan of one solve launch, filled by plan_solve (mpc_api.hip): the fields solve_key packs and format_kernel_name prints, the table row (null: not
// instantiated) and the launch geometry
struct SolvePlan {
    Family family;
    int cap;                  // row capacity (NOBST / CAP)
    int G, fact;              // one lane per stage: lanes per instance, sweep variant
    int lps;                  // stage-split and multi-wavefront: lanes per stage
    bool w2, blk2;            // stage-split: two wavefronts per SIMD, block-2 recursions
    bool masked;              // run-time obstacle count
    int level;                // 0 none, 1 REF, 2 REF + IPAR, 3 REF + IPAR + OSEL, 4 REF + IPAR + OSEL + IBND, 5 REF + IPAR + OSEL + IBND + NSQP
    const KernelRow *row;
    unsigned grid, block;
    size_t lds;
    uint32_t key() const { return family == kOneLane ? solve_key(family, cap, G, fact, 0, masked, level) : solve_key(family, cap, lps, w2, blk2, masked, level); }
};

constexpr KernelRow kSolveKernels[] = {
    // one lane per stage (G lanes per instance, sweep variant FACT: 0 systolic, 1 matrix cores, 2 row-parallel dense, 3 compact); a run-time obstacle count
    // (MASKED) and the feature levels exist for one instance per wavefront with row-parallel sweeps only
    one_lane<3, 16, 0, false, 0>(), one_lane<5, 16, 0, false, 0>(), one_lane<10, 16, 0, false, 0>(),
    one_lane<3, 16, 2, false, 0>(), one_lane<5, 16, 2, false, 0>(), one_lane<10, 16, 2, false, 0>(),
    one_lane<3, 21, 3, false, 0>(), one_lane<5, 21, 3, false, 0>(), one_lane<10, 21, 3, false, 0>(),
    one_lane<3, 32, 0, false, 0>(), one_lane<5, 32, 0, false, 0>(), one_lane<10, 32, 0, false, 0>(),
    one_lane<3, 32, 2, false, 0>(), one_lane<5, 32, 2, false, 0>(), one_lane<10, 32, 2, false, 0>(),
    one_lane<3, 64, 0, false, 0>(), one_lane<5, 64, 0, false, 0>(), one_lane<10, 64, 0, false, 0>(),
    one_lane<3, 64, 1, false, 0>(), one_lane<5, 64, 1, false, 0>(), one_lane<10, 64, 1, false, 0>(),
    one_lane<3, 64, 2, false, 0>(), one_lane<5, 64, 2, false, 0>(), one_lane<10, 64, 2, false, 0>(),
    one_lane<3, 64, 3, false, 0>(), one_lane<5, 64, 3, false, 0>(), one_lane<10, 64, 3, false, 0>(),
    one_lane<3, 64, 2, true, 0>(), one_lane<5, 64, 2, true, 0>(), one_lane<10, 64, 2, true, 0>(),
    one_lane<3, 64, 3, true, 0>(), one_lane<5, 64, 3, true, 0>(), one_lane<10, 64, 3, true, 0>(),
    one_lane<3, 64, 3, false, 1>(), one_lane<5, 64, 3, false, 1>(), one_lane<10, 64, 3, false, 1>(),
    one_lane<3, 64, 3, true, 1>(), one_lane<5, 64, 3, true, 1>(), one_lane<10, 64, 3, true, 1>(),
    one_lane<3, 64, 3, false, 2>(), one_lane<5, 64, 3, false, 2>(), one_lane<10, 64, 3, false, 2>(),
    one_lane<3, 64, 3, true, 2>(), one_lane<5, 64, 3, true, 2>(), one_lane<10, 64, 3, true, 2>(),
    one_lane<3, 64, 3, true, 3>(), one_lane<5, 64, 3, true, 3>(), one_lane<10, 64, 3, true, 3>(),
    one_lane<3, 64, 3, true, 4>(), one_lane<5, 64, 3, true, 4>(), one_lane<10, 64, 3, true, 4>(),
    one_lane<3, 64, 3, true, 5>(), one_lane<5, 64, 3, true, 5>(), one_lane<10, 64, 3, true, 5>(),
    // stage-split (LPS lanes per stage; W2: two wavefronts per SIMD; BLK2: block-2 recursions, an evidence path without feature levels); the obstacle mask
    // (level 3) is a run-time row count by nature, and the instance bounds (level 4) are built on it
    split<3, 2, false, false, false, 0>(), split<5, 2, false, false, false, 0>(), split<10, 2, false, false, false, 0>(),
    split<3, 2, true, false, false, 0>(), split<5, 2, true, false, false, 0>(), split<10, 2, true, false, false, 0>(),
    split<3, 2, false, true, false, 0>(), split<5, 2, false, true, false, 0>(), split<10, 2, false, true, false, 0>(),
    split<3, 2, false, false, true, 0>(), split<5, 2, false, false, true, 0>(), split<10, 2, false, false, true, 0>(),
    split<3, 3, false, false, false, 0>(), split<5, 3, false, false, false, 0>(), split<10, 3, false, false, false, 0>(),
    split<3, 3, true, false, false, 0>(), split<5, 3, true, false, false, 0>(), split<10, 3, true, false, false, 0>(),
    split<3, 3, false, true, false, 0>(), split<5, 3, false, true, false, 0>(), split<10, 3, false, true, false, 0>(),
    split<3, 3, false, false, true, 0>(), split<5, 3, false, false, true, 0>(), split<10, 3, false, false, true, 0>(),
    split<3, 2, false, false, false, 1>(), split<5, 2, false, false, false, 1>(), split<10, 2, false, false, false, 1>(),
    split<3, 2, true, false, false, 1>(), split<5, 2, true, false, false, 1>(), split<10, 2, true, false, false, 1>(),
    split<3, 2, false, true, false, 1>(), split<5, 2, false, true, false, 1>(), split<10, 2, false, true, false, 1>(),
    split<3, 3, false, false, false, 1>(), split<5, 3, false, false, false, 1>(), split<10, 3, false, false, false, 1>(),
    split<3, 3, true, false, false, 1>(), split<5, 3, true, false, false, 1>(), split<10, 3, true, false, false, 1>(),
    split<3, 3, false, true, false, 1>(), split<5, 3, false, true, false, 1>(), split<10, 3, false, true, false, 1>(),
    split<3, 2, false, false, false, 2>(), split<5, 2, false, false, false, 2>(), split<10, 2, false, false, false, 2>(),
    split<3, 2, true, false, false, 2>(), split<5, 2, true, false, false, 2>(), split<10, 2, true, false, false, 2>(),
    split<3, 2, false, true, false, 2>(), split<5, 2, false, true, false, 2>(), split<10, 2, false, true, false, 2>(),
    split<3, 3, false, false, false, 2>(), split<5, 3, false, false, false, 2>(), split<10, 3, false, false, false, 2>(),
    split<3, 3, true, false, false, 2>(), split<5, 3, true, false, false, 2>(), split<10, 3, true, false, false, 2>(),
    split<3, 3, false, true, false, 2>(), split<5, 3, false, true, false, 2>(), split<10, 3, false, true, false, 2>(),
    split<3, 2, false, true, false, 3>(), split<5, 2, false, true, false, 3>(), split<10, 2, false, true, false, 3>(),
    split<3, 3, false, true, false, 3>(), split<5, 3, false, true, false, 3>(), split<10, 3, false, true, false, 3>(),
    split<3, 2, false, true, false, 4>(), split<5, 2, false, true, false, 4>(), split<10, 2, false, true, false, 4>(),
    split<3, 3, false, true, false, 4>(), split<5, 3, false, true, false, 4>(), split<10, 3, false, true, false, 4>(),
    // ... and the SQP loop (level 5) on them
    split<3, 2, false, true, false, 5>(), split<5, 2, false, true, false, 5>(), split<10, 2, false, true, false, 5>(),
    split<3, 3, false, true, false, 5>(), split<5, 3, false, true, false, 5>(), split<10, 3, false, true, false, 5>(),
    // multi-wavefront, 11 .. 32 obstacles
    wide<20, false, 0>(), wide<32, false, 0>(),
    wide<20, true, 0>(), wide<32, true, 0>(),
    wide<20, false, 1>(), wide<32, false, 1>(),
    wide<20, true, 1>(), wide<32, true, 1>(),
    wide<20, false, 2>(), wide<32, false, 2>(),
    wide<20, true, 2>(), wide<32, true, 2>(),
    wide<20, true, 3>(), wide<32, true, 3>(),
    wide<20, true, 4>(), wide<32, true, 4>(),
    wide<20, true, 5>(), wide<32, true, 5>(),
};

constexpr int kSolveKernelCount = sizeof(kSolveKernels) / sizeof(kSolveKernels[0]);

constexpr bool solve_keys_distinct()
{
    for (int i = 0; i < kSolveKernelCount; i++)
        for (int j = 0; j < i; j++)
            if (kSolveKernels[i].key == kSolveKernels[j].key) return false;
    return true;
}
static_assert(solve_keys_distinct(), "two rows of kSolveKernels have the same key");

inline const KernelRow *find_solve_kernel(uint32_t key)
{
    for (const KernelRow &r : kSolveKernels)
        if (r.key == key) return &r;
    return nullptr;
}

// the instantiation as rocprofv3 prints it (without the namespace): the family's own template arguments, then one `, true` per feature level
inline void format_kernel_name(const SolvePlan &q, char *buf, size_t len)
{
    const char *tf[2] = {"false", "true"}, *level[6] = {"", ", true", ", true, true", ", true, true, true", ", true, true, true, true", ", true, true, true, true, true"};
    if (q.family == kWide) snprintf(buf, len, "rti_wide_kernel<%d, %d, %s%s>", q.cap, q.lps, tf[q.masked], level[q.level]);
    else if (q.family == kSplit) snprintf(buf, len, "rti_split_kernel<%d, %d, %s, %s, %s%s>", q.cap, q.lps, tf[q.w2], tf[q.masked], tf[q.blk2], level[q.level]);
    else snprintf(buf, len, "rti_solve_kernel<%d, %d, %d, %s%s>", q.cap, q.G, q.fact, tf[q.masked], level[q.level]);
}

}  // namespace mpc
