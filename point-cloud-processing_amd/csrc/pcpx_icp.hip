// pcpx_icp.hip -- iterative closest point on the indexed cloud (include/pcpx_icp.h): the exact nearest indexed
// point of every source point under a pose, and the loop around it, enqueued whole.  An eighth form of the leaf-direct sphere walk of
// pcpx_device.h: its pair test is "nearer than what the lane holds, or as near with a lower index", and the lane's radius shrinks to
// every partner it finds.
//   k_icp_moved       the source under a pose, rounded to float32: what the curve sort of pcpx_prep.hip orders, once per call
//   k_nearest_posed   one wavefront per 64 consecutive positions of that order, one lane per source point
//   k_icp_init / k_icp_decide / k_icp_commit / k_icp_finish   the loop's rules on a block of device words, a thread or a wave each
//   k_fixed_partial / k_fixed_final (pcpx_fixed_sum.h) over PlaneSystem, k_plane_solve   the point-to-plane step: 29 float64 sums in
//                     the fits' fixed order, Cholesky
// The point-to-point step is the rigid fit of pcpx_register.hip through fit_pairs_device: the same kernels, so the same bits.
// icp_loop_device runs the same loop around a caller's sums in the point-to-plane layout (pcpx_gicp.hip: the plane-to-plane step).
#include "pcpx_device.h"
#include "pcpx_fixed_sum.h"
#include "pcpx_icp.h"
#include "pcpx_lease.h"
#include "pcpx_plane_solve.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

namespace pcpx {

namespace {

constexpr u32 ICP_BLOCK = 256;
constexpr u32 ICP_NONE = PCPX_ICP_NONE;
// From the second round on a lane may start from (d2 to its previous partner, that partner) instead of (radius^2, none): the previous
// partner is a candidate like any other, so the minimum of (d2, index) and with it every bit is unchanged; it costs one gather per
// lane.  Shipped as measured; pcpx_debug_set "icp_previous_start" overrides it for the A/B.
constexpr bool ICP_PREVIOUS_START = true;
// k_nearest_posed's two counts of a round are spread over ICP_SLOTS words ICP_SLOT_STRIDE words apart, wave g adding to slot
// g mod ICP_SLOTS: 15 625 atomics of a million-point source on ONE word took twice as long as the search itself.
constexpr u32 ICP_SLOTS = 64, ICP_SLOT_STRIDE = 32;
constexpr u32 PLANE_TERMS = PLANE_A_TERMS + PLANE_B_TERMS + 2, PLANE_STRIDE = 32;  // A, b, sum rho^2, rows


// The words of a loop on the device.  done: every kernel of a later round reads it first and returns.  fit_count: the number of
// correspondences the fit's kernels see -- m while the loop runs, 0 once it has stopped, so that they pass over nothing and stay
// what they are for their other callers.  A round's step writes cand; k_icp_commit makes it the pose only while done is clear.
struct IcpState {
    u32 done, status, iterations, last_count;
    u32 last_buffer, degenerate, pad0[2];
    u64 fit_count, pad;
    double pose[16], cand[16];
    double rms_cand, pad2[3];
    double plane[PLANE_STRIDE];
    u32 slots[ICP_SLOTS * ICP_SLOT_STRIDE];  // [slot][0]: rows WITHOUT a partner, [slot][1]: rows that differ from the round before
};
static_assert(sizeof(IcpState) % 8 == 0, "doubles stay aligned");

struct Pose12 {
    double v[12];
};

// y = T s of pcpx_icp.h: float64, each operation rounded on its own, in the written order
__device__ __forceinline__ void moved_point(const Pose12& T, float s0, float s1, float s2, double (&y)[3])
{
    const double a = s0, b = s1, c = s2;
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = ((T.v[4 * r] * a + T.v[4 * r + 1] * b) + T.v[4 * r + 2] * c) + T.v[4 * r + 3];
}
// the pose as a wave-uniform load; null: the identity matrix
__device__ __forceinline__ Pose12 load_pose(const double* pose)
{
    if (pose) return load_const(reinterpret_cast<const Pose12*>(pose));
    return Pose12{{1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0}};
}

__global__ __launch_bounds__(ICP_BLOCK) void k_icp_moved(const float* __restrict__ s, u32 m, const double* __restrict__ pose, float* __restrict__ y32)
{
    const u32 i = blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const Pose12 T = load_pose(pose);
    double y[3];
    moved_point(T, s[3ull * i], s[3ull * i + 1], s[3ull * i + 2], y);
#pragma unroll
    for (int r = 0; r < 3; ++r) y32[3ull * i + r] = static_cast<float>(y[r]);
}

// One wave per 64 consecutive positions of the source order (order[p] = the source row at position p; null: p itself), one lane per
// source point.  The lane moves its point once (9 multiplications and 9 additions in float64) and carries (r2, best), which start at
// (radius^2, none): a point is taken when it is nearer than r2, or as near with a lower input index, and r2 shrinks to it.  The
// box test is `<=`: a point at exactly r2 with a lower index must still be seen, and the first hit at radius^2 passes the same test
// because every index is below 2^32 - 1.  Pruning relies, as every sphere form of the walk does, on the float32 box_d2 never
// exceeding the sq3 of a point inside the box (pcpx_box_bound.h).  The result is the minimum of (d2, index) over the sphere, so it
// depends neither on the order of the leaves nor on the source order.  No LDS, no floating-point reduction; the loop's two counts
// ("has no partner", "differs from the round before") are one ballot each and, where the count is not zero, one integer atomic per
// wave on the wave's slot: integers, so the order does not matter.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_nearest_posed(TreeView t, u32 group_end, u32 m, const float* __restrict__ s,
                                                                       const u32* __restrict__ order, const double* __restrict__ pose, float radius,
                                                                       const u32* __restrict__ done, u32* __restrict__ partner, float* __restrict__ out_d2,
                                                                       uint2* __restrict__ pairs, const uint2* __restrict__ previous,
                                                                       const float* __restrict__ start_xyz, u32* __restrict__ counters)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    if (done && load_const(done) != 0u) return;
    const u32 p = g * GROUP + lane;
    const bool active = p < m;
    u32 row = 0;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (active) {
        row = order ? order[p] : p;
        s0 = s[3ull * row], s1 = s[3ull * row + 1], s2 = s[3ull * row + 2];
    }
    const Pose12 T = load_pose(pose);
    double y[3];
    moved_point(T, s0, s1, s2, y);
    const float qx = static_cast<float>(y[0]), qy = static_cast<float>(y[1]), qz = static_cast<float>(y[2]);
    float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    u32 best = ICP_NONE;
    if (start_xyz && active) {  // the previous partner first (the target by input row): an indexed point, its d2 formed as the walk forms it
        const u32 j = previous[row].y;
        if (j != ICP_NONE) {
            const float dx = start_xyz[3ull * j] - qx, dy = start_xyz[3ull * j + 1] - qy, dz = start_xyz[3ull * j + 2] - qz;
            const float d2 = sq3(dx, dy, dz);
            if (d2 <= r2) {
                r2 = d2;
                best = j;
            }
        }
    }
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };  // (false for a NaN query)
    walk_needed_leaves<false>(t, need, [&](const u32, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const float d2 = sq3(dx, dy, dz);
            if (d2 < r2 || (d2 == r2 && lf.id[j] < best)) {  // (a NaN padding point fails both)
                r2 = d2;
                best = lf.id[j];
            }
        }
    });
    if (active) {
        if (partner) partner[row] = best;
        if (out_d2) out_d2[row] = best != ICP_NONE ? r2 : std::numeric_limits<float>::infinity();
        if (pairs) pairs[row] = uint2{row, best};
    }
    if (counters) {
        const bool differs = active && previous && previous[row].y != best;  // (the first round has nothing to differ from)
        const u32 none = static_cast<u32>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(active && best == ICP_NONE)));
        const u32 dif = static_cast<u32>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(differs)));
        u32* slot = counters + (g % ICP_SLOTS) * ICP_SLOT_STRIDE;
        if (lane == 0) {
            if (none) atomicAdd(slot, none);
            if (dif) atomicAdd(slot + 1, dif);
        }
    }
}

// ---- the loop's rules (pcpx_icp.h, steps 2-6) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_init(IcpState* __restrict__ st, const double* __restrict__ pose, u32 m, u32 max_iterations,
                                                       u32* __restrict__ count_trace, double* __restrict__ rms_trace)
{
    for (u32 k = threadIdx.x; k < max_iterations; k += ICP_BLOCK) {
        if (count_trace) count_trace[k] = 0u;
        if (rms_trace) rms_trace[k] = std::numeric_limits<double>::quiet_NaN();
    }
    for (u32 j = threadIdx.x; j < ICP_SLOTS * ICP_SLOT_STRIDE; j += ICP_BLOCK) st->slots[j] = 0u;
    if (threadIdx.x != 0) return;
    st->done = st->status = st->iterations = st->last_count = 0u;
    st->last_buffer = st->degenerate = st->pad0[0] = st->pad0[1] = 0u;
    st->fit_count = m;
    st->pad = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        st->pose[j] = pose ? pose[j] : ((j % 5 == 0) ? 1.0 : 0.0);
        st->cand[j] = 0.0;
    }
    st->rms_cand = std::numeric_limits<double>::quiet_NaN();
}

// after step 1 of round k: steps 2 to 4.  One wave: lane s takes slot s's two counts and clears them, the wave adds them up.
__global__ __launch_bounds__(64) void k_icp_decide(IcpState* __restrict__ st, u32 k, u32 min_count, u32 m)
{
    static_assert(ICP_SLOTS == 64, "one slot per lane");
    if (st->done) return;
    u32* slot = st->slots + threadIdx.x * ICP_SLOT_STRIDE;
    u32 none = slot[0], differ = slot[1];
    slot[0] = 0u;
    slot[1] = 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        none += __shfl_xor(none, off);
        differ += __shfl_xor(differ, off);
    }
    if (threadIdx.x != 0) return;
    const u32 count = m - none;
    st->last_count = count;
    st->last_buffer = k & 1u;
    if (k > 0u && differ == 0u) {
        st->status = PCPX_ICP_CONVERGED;
        st->done = 1u;
    } else if (count < min_count) {
        st->status = PCPX_ICP_STARVED;
        st->done = 1u;
    }
    if (st->done) st->fit_count = 0;
}

// after step 5 of round k: the candidate becomes the pose, the traces get their entries, step 6
__global__ __launch_bounds__(64) void k_icp_commit(IcpState* __restrict__ st, u32 k, u32 max_iterations, u32* __restrict__ count_trace,
                                                  double* __restrict__ rms_trace)
{
    if (threadIdx.x != 0 || st->done) return;
    if (st->degenerate) {
        st->status = PCPX_ICP_DEGENERATE;
        st->done = 1u;
        st->fit_count = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) st->pose[j] = st->cand[j];
    if (count_trace) count_trace[k] = st->last_count;
    if (rms_trace) rms_trace[k] = st->rms_cand;
    st->iterations = k + 1u;
    if (k + 1u == max_iterations) {
        st->status = PCPX_ICP_EXHAUSTED;
        st->done = 1u;
        st->fit_count = 0;
    }
}

// the outputs: the first thread the words and the transform, everybody the last partner list
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_finish(const IcpState* __restrict__ st, const uint2* __restrict__ pairs0, const uint2* __restrict__ pairs1,
                                                         u32 m, double* __restrict__ transform, u32* __restrict__ status, u32* __restrict__ iterations,
                                                         u32* __restrict__ last_count, u32* __restrict__ partner)
{
    const u32 i = blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (partner && i < m) partner[i] = (st->last_buffer ? pairs1 : pairs0)[i].y;
    if (i != 0) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) transform[j] = st->pose[j];
    if (status) *status = st->status;
    if (iterations) *iterations = st->iterations;
    if (last_count) *last_count = st->last_count;
}

// ---- the point-to-plane step ---------------------------------------------------------------------------------------------------------
struct PlaneIn {
    const float* s;        // the source
    const float* xyz;      // the target by input row
    const float* normals;  // its normals by input row
    const uint2* pairs;    // {i, partner of i}, m of them
    u32 m, n_in;
    double o[3];
};

// The sums of the normal equations over the rows that have a partner, in pcpx_fixed_sum.h's order; the totals go to st->plane.  Once
// the loop has stopped there are no rows: the launches still run, and leave zeros.
struct PlaneSystem {
    static constexpr int TERMS = PLANE_TERMS, STRIDE = PLANE_STRIDE;
    PlaneIn in;
    IcpState* st;
    Pose12 T;  // (items() leaves the round's pose here for add())
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ u32 items()
    {
#pragma unroll
        for (int j = 0; j < 12; ++j) T.v[j] = st->pose[j];
        return st->done ? 0u : in.m;
    }
    __device__ __forceinline__ void add(u32 j, double (&acc)[TERMS]) const
    {
        const u32 target = in.pairs[j].y;
        if (target >= in.n_in) return;  // (no partner)
        const float n0 = in.normals[3ull * target], n1 = in.normals[3ull * target + 1], n2 = in.normals[3ull * target + 2];
        if (!(std::isfinite(n0) && std::isfinite(n1) && std::isfinite(n2))) return;
        double y[3];
        moved_point(T, in.s[3ull * j], in.s[3ull * j + 1], in.s[3ull * j + 2], y);
        const double e0 = y[0] - static_cast<double>(in.xyz[3ull * target]), e1 = y[1] - static_cast<double>(in.xyz[3ull * target + 1]),
                     e2 = y[2] - static_cast<double>(in.xyz[3ull * target + 2]);
        const double u0 = y[0] - in.o[0], u1 = y[1] - in.o[1], u2 = y[2] - in.o[2];
        double J[6];
        J[3] = n0, J[4] = n1, J[5] = n2;
        const double rho = (e0 * J[3] + e1 * J[4]) + e2 * J[5];
        J[0] = u1 * J[5] - u2 * J[4];
        J[1] = u2 * J[3] - u0 * J[5];
        J[2] = u0 * J[4] - u1 * J[3];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) acc[plane_at(r, c)] += J[r] * J[c];
            acc[PLANE_A_TERMS + r] -= rho * J[r];
        }
        acc[PLANE_A_TERMS + PLANE_B_TERMS] += rho * rho;
        acc[PLANE_A_TERMS + PLANE_B_TERMS + 1] += 1.0;
    }
    __device__ __forceinline__ void finish(u32 term, double sum) const { st->plane[term] = sum; }
};

// one thread: Cholesky, the Cayley step and the new pose into cand, or the degenerate word
__global__ __launch_bounds__(64) void k_plane_solve(IcpState* __restrict__ st, double o0, double o1, double o2)
{
    if (threadIdx.x != 0 || st->done) return;
    double a[PLANE_A_TERMS], b[PLANE_B_TERMS], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < PLANE_A_TERMS; ++i) a[i] = st->plane[i];
#pragma unroll
    for (int i = 0; i < PLANE_B_TERMS; ++i) b[i] = st->plane[PLANE_A_TERMS + i];
    if (!plane_cholesky(a, b, x)) {
        st->degenerate = 1u;
        return;
    }
    const double o[3] = {o0, o1, o2};
    double pose[16], out[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) pose[j] = st->pose[j];
    plane_compose(pose, o, x, out);
#pragma unroll
    for (int j = 0; j < 16; ++j) st->cand[j] = out[j];
    st->rms_cand = std::sqrt(st->plane[PLANE_A_TERMS + PLANE_B_TERMS] / st->plane[PLANE_A_TERMS + PLANE_B_TERMS + 1]);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
int check_nearest(const char* what, const void* s, u64 m, float radius)
{
    if (!(radius >= 0.f) || radius == std::numeric_limits<float>::infinity()) {  // (false for a NaN)
        set_error("%s: the radius must be finite and >= 0 (got %g)", what, static_cast<double>(radius));
        return PCPX_ERR_INVALID;
    }
    if (m >= 0xFFFFFFFFull) {
        set_error("%s: m = %llu source points: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(m));
        return PCPX_ERR_INVALID;
    }
    if (!s && m) {
        set_error("%s: the source array is NULL with m = %llu", what, static_cast<unsigned long long>(m));
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_iterations(const char* what, u32 max_iterations)
{
    if (max_iterations < 1u || max_iterations > PCPX_ICP_MAX_ITERATIONS) {
        set_error("%s: max_iterations = %u is not in 1 .. %u", what, max_iterations, PCPX_ICP_MAX_ITERATIONS);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_transform(const char* what, const void* transform)
{
    if (!transform) {
        set_error("%s: the transform array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_loop(const char* what, u32 max_iterations, u32 flags, const void* normals, const void* transform)
{
    if (const int st = check_iterations(what, max_iterations)) return st;
    if (flags & ~PCPX_ICP_POINT_TO_PLANE) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~PCPX_ICP_POINT_TO_PLANE);
        return PCPX_ERR_INVALID;
    }
    if ((flags & PCPX_ICP_POINT_TO_PLANE) && !normals) {
        set_error("%s: PCPX_ICP_POINT_TO_PLANE without normals", what);
        return PCPX_ERR_INVALID;
    }
    if (!(flags & PCPX_ICP_POINT_TO_PLANE) && normals) {
        set_error("%s: normals without PCPX_ICP_POINT_TO_PLANE", what);
        return PCPX_ERR_INVALID;
    }
    return check_transform(what, transform);
}

// the source order: the curve sort of the moved points by the machinery of pcpx_prep.hip, copied out of the handle's scratch (which
// the next call on the handle reuses) into `order`.  y32: room for m x 3 floats.
int make_source_order(Index& ix, const float* d_s, u32 m, const double* d_pose, float* y32, u32* order)
{
    int st;
    k_icp_moved<<<blocks_of(m, ICP_BLOCK), ICP_BLOCK, 0, ix.stream>>>(d_s, m, d_pose, y32);
    PCPX_HIP(hipGetLastError());
    QueryView qv;
    if ((st = prepare_queries(ix, y32, m, qv)) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(order, qv.row, static_cast<size_t>(m) * sizeof(u32), hipMemcpyDeviceToDevice, ix.stream));
    return PCPX_OK;
}

// what a call takes from the lease
struct IcpScratch {
    size_t state = 0, y32 = 0, order = 0, pairs0 = 0, pairs1 = 0, fit = 0, plane = 0, bytes = 0;
    IcpScratch(u64 m, bool loop)
    {
        Carve c;
        y32 = c.take(m * 3 * sizeof(float));
        order = c.take(m * sizeof(u32));
        if (loop) {
            state = c.take(sizeof(IcpState));
            pairs0 = c.take(m * sizeof(uint2));
            pairs1 = c.take(m * sizeof(uint2));
            fit = c.take(fit_scratch_bytes());
            plane = c.take(static_cast<u64>(FIT_BLOCKS) * PLANE_STRIDE * sizeof(double));
        }
        bytes = c.bytes() ? c.bytes() : 256;
    }
};

// a lease of the device's pool for a call on a handle: the call returns before its kernels have run, so its block may go back only
// once the handle's stream has passed it (pcpx_lease.h)
template <class Body>
int with_lease(Index& ix, size_t bytes, Body&& body)
{
    if (ix.device < 0 || ix.device >= LEASE_MAX_DEVICES) {
        set_error("pcpx_icp: device %d is beyond the lease's %d", ix.device, LEASE_MAX_DEVICES);
        return PCPX_ERR_UNSUPPORTED;
    }
    DeviceShared& sh = shared_of(ix.device);
    std::lock_guard<std::mutex> lock(sh.mu);
    return leased(sh, ix.device, ix.stream, bytes, body);
}

int nearest_device(Index& ix, const float* d_s, u64 m64, const double* d_pose, float radius, u32* d_partner, float* d_d2)
{
    if (m64 == 0) return PCPX_OK;
    const u32 m = static_cast<u32>(m64);
    const IcpScratch L(m, false);
    return with_lease(ix, L.bytes, [&](char* base) -> int {
        int st;
        u32* order = nullptr;
        if (ix.n > 0) {  // (an empty index has no curve; every row is without a partner in any order)
            order = reinterpret_cast<u32*>(base + L.order);
            if ((st = make_source_order(ix, d_s, m, d_pose, reinterpret_cast<float*>(base + L.y32), order)) != PCPX_OK) return st;
        }
        const u32 groups = blocks_of(m, GROUP);
        k_nearest_posed<<<grid_for_groups(groups), 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), groups, m, d_s, order, d_pose, radius, nullptr, d_partner,
                                                                                       d_d2, nullptr, nullptr, nullptr, nullptr);
        PCPX_HIP(hipGetLastError());
        return PCPX_OK;
    });
}

using LoopOut = IcpLoopOut;

// custom: the round's sums by the caller's step (icp_loop_device) instead of one of the two modes of `flags`
int icp_device(Index& ix, const float* d_s, u64 m64, const double* d_pose, float radius, u32 max_iterations, u32 flags, const float* d_normals,
               const LoopOut& out, const char* what = "pcpx_icp_rigid", const IcpSumsStep* custom = nullptr)
{
    const bool plane = (flags & PCPX_ICP_POINT_TO_PLANE) != 0u;
    if (ix.n_in && !ix.d_xyz) {
        set_error("%s: the handle keeps no copy of its cloud", what);
        return PCPX_ERR_UNSUPPORTED;
    }
    const u32 m = static_cast<u32>(m64);
    const IcpScratch L(m, true);
    return with_lease(ix, L.bytes, [&](char* base) -> int {
        int st;
        hipStream_t s = ix.stream;
        IcpState* state = reinterpret_cast<IcpState*>(base + L.state);
        float* y32 = reinterpret_cast<float*>(base + L.y32);
        u32* order = (ix.n > 0 && m > 0) ? reinterpret_cast<u32*>(base + L.order) : nullptr;
        uint2* pairs[2] = {reinterpret_cast<uint2*>(base + L.pairs0), reinterpret_cast<uint2*>(base + L.pairs1)};
        double* plane_partial = reinterpret_cast<double*>(base + L.plane);
        const double o[3] = {(static_cast<double>(ix.bbox[0]) + static_cast<double>(ix.bbox[3])) / 2.0,
                             (static_cast<double>(ix.bbox[1]) + static_cast<double>(ix.bbox[4])) / 2.0,
                             (static_cast<double>(ix.bbox[2]) + static_cast<double>(ix.bbox[5])) / 2.0};
        const u32 groups = blocks_of(m, GROUP);
        const TreeView t = ix.view();
        const bool previous_start = ix.tuning.icp_previous_start < 0 ? ICP_PREVIOUS_START : ix.tuning.icp_previous_start != 0;
        k_icp_init<<<1, ICP_BLOCK, 0, s>>>(state, d_pose, m, max_iterations, out.count_trace, out.rms_trace);
        PCPX_HIP(hipGetLastError());
        if (order && (st = make_source_order(ix, d_s, m, d_pose, y32, order)) != PCPX_OK) return st;
        for (u32 k = 0; k < max_iterations; ++k) {
            if (order && k > 0 && ix.tuning.icp_resort && (st = make_source_order(ix, d_s, m, state->pose, y32, order)) != PCPX_OK) return st;
            if (m > 0)
                k_nearest_posed<<<grid_for_groups(groups), 64 * WAVES_PER_BLOCK, 0, s>>>(t, groups, m, d_s, order, state->pose, radius, &state->done, nullptr,
                                                                                       nullptr, pairs[k & 1u], k > 0 ? pairs[(k - 1u) & 1u] : nullptr,
                                                                                       k > 0 && previous_start ? ix.d_xyz : nullptr, state->slots);
            k_icp_decide<<<1, 64, 0, s>>>(state, k, custom ? custom->min_count : plane ? 6u : 3u, m);
            if (custom) {
                if ((st = custom->enqueue(custom->ctx, state->pose, &state->done, state->plane, reinterpret_cast<const u32*>(pairs[k & 1u]), plane_partial,
                                          s)) != PCPX_OK)
                    return st;
                k_plane_solve<<<1, 64, 0, s>>>(state, o[0], o[1], o[2]);
            } else if (plane) {
                const PlaneIn in{d_s, ix.d_xyz, d_normals, pairs[k & 1u], m, static_cast<u32>(ix.n_in), {o[0], o[1], o[2]}};
                fixed_sum(PlaneSystem{in, state, {}}, plane_partial, s);
                k_plane_solve<<<1, 64, 0, s>>>(state, o[0], o[1], o[2]);
            } else if ((st = fit_pairs_device(d_s, m, ix.d_xyz, static_cast<u32>(ix.n_in), reinterpret_cast<const u32*>(pairs[k & 1u]), m,
                                              &state->fit_count, base + L.fit, state->pose, state->cand, &state->rms_cand, s)) != PCPX_OK) {
                return st;
            }
            k_icp_commit<<<1, 64, 0, s>>>(state, k, max_iterations, out.count_trace, out.rms_trace);
            PCPX_HIP(hipGetLastError());
        }
        k_icp_finish<<<out.partner && m ? blocks_of(m, ICP_BLOCK) : 1u, ICP_BLOCK, 0, s>>>(state, pairs[0], pairs[1], m, out.transform, out.status,
                                                                                         out.iterations, out.last_count, out.partner);
        PCPX_HIP(hipGetLastError());
        return PCPX_OK;
    });
}

// One interval of the PCPX_K_RANGE family for the whole call: what the call launches through other modules books nothing of its own.
template <class Body>
int booked_as_one_range_interval(Index& ix, Body&& body)
{
    ProfileScope prof(ix, PCPX_K_RANGE);
    const bool profiling = ix.profiling;
    ix.profiling = false;
    const int st = body();
    ix.profiling = profiling;
    return st;
}

}  // namespace

int icp_check_arguments(const char* what, const void* s, u64 m, float radius, u32 max_iterations, const void* transform)
{
    int st = check_nearest(what, s, m, radius);
    if (st != PCPX_OK || (st = check_iterations(what, max_iterations)) != PCPX_OK) return st;
    return check_transform(what, transform);
}

int icp_loop_device(Index& ix, const char* what, const float* d_s, u64 m, const double* d_pose, float radius, u32 max_iterations,
                    const IcpSumsStep& step, const IcpLoopOut& out)
{
    return booked_as_one_range_interval(ix, [&] { return icp_device(ix, d_s, m, d_pose, radius, max_iterations, 0u, nullptr, out, what, &step); });
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_nearest_posed_dev(pcpx_index* h, const float* d_s, uint64_t m, const double* d_opt_pose, float radius, uint32_t* d_out_partner,
                           float* d_opt_out_d2)
{
    static const char* what = "pcpx_nearest_posed_dev";
    int st = check_nearest(what, d_s, m, radius);
    if (st != PCPX_OK) return st;
    if (!d_out_partner) {
        set_error("%s: the partner array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        return booked_as_one_range_interval(*ix, [&] { return nearest_device(*ix, d_s, m, d_opt_pose, radius, d_out_partner, d_opt_out_d2); });
    });
}

int pcpx_nearest_posed(pcpx_index* h, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t* out_partner, float* opt_out_d2)
{
    static const char* what = "pcpx_nearest_posed";
    int st = check_nearest(what, s, m, radius);
    if (st != PCPX_OK) return st;
    if (!out_partner) {
        set_error("%s: the partner array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        if (m == 0) return PCPX_OK;
        int r;
        DevBuf ds(ix->pool), dpose(ix->pool), dpart(ix->pool), dd2(ix->pool);
        if ((r = ds.alloc(m * 3 * sizeof(float))) != PCPX_OK || (r = dpart.alloc(m * sizeof(u32))) != PCPX_OK ||
            (opt_pose && (r = dpose.alloc(16 * sizeof(double))) != PCPX_OK) || (opt_out_d2 && (r = dd2.alloc(m * sizeof(float))) != PCPX_OK))
            return r;
        if ((r = upload_pageable(ds.p, s, m * 3 * sizeof(float), ix->stream)) != PCPX_OK) return r;
        if (opt_pose && (r = upload_pageable(dpose.p, opt_pose, 16 * sizeof(double), ix->stream)) != PCPX_OK) return r;
        if ((r = booked_as_one_range_interval(*ix, [&] {
                 return nearest_device(*ix, ds.as<float>(), m, dpose.as<double>(), radius, dpart.as<u32>(), dd2.as<float>());
             })) != PCPX_OK)
            return r;
        PCPX_HIP(hipMemcpyAsync(out_partner, dpart.p, m * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
        if (opt_out_d2) PCPX_HIP(hipMemcpyAsync(opt_out_d2, dd2.p, m * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
        PCPX_HIP(hipStreamSynchronize(ix->stream));
        return PCPX_OK;
    });
}

int pcpx_icp_rigid_dev(pcpx_index* h, const float* d_s, uint64_t m, const double* d_opt_pose, float radius, uint32_t max_iterations, uint32_t flags,
                       const float* d_opt_normals, double* d_out_transform, uint32_t* d_opt_out_status, uint32_t* d_opt_out_iterations,
                       uint32_t* d_opt_out_last_count, uint32_t* d_opt_out_count_trace, double* d_opt_out_rms_trace, uint32_t* d_opt_out_partner)
{
    static const char* what = "pcpx_icp_rigid_dev";
    int st = check_nearest(what, d_s, m, radius);
    if (st != PCPX_OK || (st = check_loop(what, max_iterations, flags, d_opt_normals, d_out_transform)) != PCPX_OK) return st;
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        const LoopOut out{d_out_transform, d_opt_out_status, d_opt_out_iterations, d_opt_out_last_count, d_opt_out_count_trace, d_opt_out_rms_trace,
                          d_opt_out_partner};
        return booked_as_one_range_interval(*ix, [&] { return icp_device(*ix, d_s, m, d_opt_pose, radius, max_iterations, flags, d_opt_normals, out); });
    });
}

int pcpx_icp_rigid(pcpx_index* h, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t max_iterations, uint32_t flags,
                   const float* opt_normals, double* out_transform, uint32_t* opt_out_status, uint32_t* opt_out_iterations,
                   uint32_t* opt_out_last_count, uint32_t* opt_out_count_trace, double* opt_out_rms_trace, uint32_t* opt_out_partner)
{
    static const char* what = "pcpx_icp_rigid";
    int st = check_nearest(what, s, m, radius);
    if (st != PCPX_OK || (st = check_loop(what, max_iterations, flags, opt_normals, out_transform)) != PCPX_OK) return st;
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        // the small outputs as one block: the transform, the rms trace, then the words and the count trace
        struct Small {
            double transform[16], rms[PCPX_ICP_MAX_ITERATIONS];
            u32 status, iterations, last_count, pad, count[PCPX_ICP_MAX_ITERATIONS];
        };
        int r;
        DevBuf ds(ix->pool), dpose(ix->pool), dnrm(ix->pool), dpart(ix->pool), dsmall(ix->pool);
        std::vector<Small> host(1);
        if ((m && (r = ds.alloc(m * 3 * sizeof(float))) != PCPX_OK) || (opt_pose && (r = dpose.alloc(16 * sizeof(double))) != PCPX_OK) ||
            (opt_normals && ix->n_in && (r = dnrm.alloc(ix->n_in * 3 * sizeof(float))) != PCPX_OK) ||
            (opt_out_partner && m && (r = dpart.alloc(m * sizeof(u32))) != PCPX_OK) || (r = dsmall.alloc(sizeof(Small))) != PCPX_OK)
            return r;
        if (m && (r = upload_pageable(ds.p, s, m * 3 * sizeof(float), ix->stream)) != PCPX_OK) return r;
        if (opt_pose && (r = upload_pageable(dpose.p, opt_pose, 16 * sizeof(double), ix->stream)) != PCPX_OK) return r;
        if (dnrm.p && (r = upload_pageable(dnrm.p, opt_normals, ix->n_in * 3 * sizeof(float), ix->stream)) != PCPX_OK) return r;
        Small* d = dsmall.as<Small>();
        // (an empty target with the flag: the address only says "point to plane", nothing is read through it)
        const float* normals = opt_normals ? (dnrm.p ? dnrm.as<float>() : reinterpret_cast<const float*>(d)) : nullptr;
        const LoopOut out{d->transform, &d->status, &d->iterations, &d->last_count, d->count, d->rms, dpart.as<u32>()};
        if ((r = booked_as_one_range_interval(*ix, [&] {
                 return icp_device(*ix, ds.as<float>(), m, dpose.as<double>(), radius, max_iterations, flags, normals, out);
             })) != PCPX_OK)
            return r;
        PCPX_HIP(hipMemcpyAsync(host.data(), d, sizeof(Small), hipMemcpyDeviceToHost, ix->stream));
        if (dpart.p) PCPX_HIP(hipMemcpyAsync(opt_out_partner, dpart.p, m * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
        PCPX_HIP(hipStreamSynchronize(ix->stream));
        const Small& o = host[0];
        std::copy(o.transform, o.transform + 16, out_transform);
        if (opt_out_status) *opt_out_status = o.status;
        if (opt_out_iterations) *opt_out_iterations = o.iterations;
        if (opt_out_last_count) *opt_out_last_count = o.last_count;
        if (opt_out_count_trace) std::copy(o.count, o.count + max_iterations, opt_out_count_trace);
        if (opt_out_rms_trace) std::copy(o.rms, o.rms + max_iterations, opt_out_rms_trace);
        return PCPX_OK;
    });
}

}  // extern "C"
