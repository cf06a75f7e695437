// pcpx_register.hip -- rigid registration from correspondences (include/pcpx_register.h): a fixed number of
// three-pair hypotheses, each scored against all correspondences, and the least-squares rigid fit.  The hot path has the form of
// k_match (pcpx_match.hip): one lane per hypothesis with its rotation and translation in registers, a correspondence's record a
// wave-uniform scalar load.  No LDS, no atomics but one integer maximum per wave, nothing between workgroups:
//   k_reg_pack       correspondences -> 32-byte records (p - o_p, q - o_q, two zeros), NaN-marked where not usable
//   k_ransac_count   one wavefront per (64 consecutive hypotheses, one segment of the records): one count per lane
//   k_ransac_best    one thread per hypothesis over its segments' counts; the best key by a wave reduction and one atomicMax
//   k_ransac_emit    the winner rebuilt by the same device function: its transform, and the inlier flag of every record;
//                    pcpx_scan.h and k_reg_compact write the inliers' positions
//   k_fixed_partial / k_fixed_final (pcpx_fixed_sum.h) over RigidSum<1..3>, k_fit_solve   the float64 sums of the rigid fit in the
//                    fixed order, and Horn's closed form
#include "pcpx_device.h"
#include "pcpx_horn.h"
#include "pcpx_lease.h"
#include "pcpx_ransac.h"
#include "pcpx_register.h"
#include "pcpx_scan.h"

#include <algorithm>
#include <limits>

namespace pcpx {

namespace {

constexpr u32 RG_WAVES = 4;    // waves of a k_ransac_count block: four consecutive hypothesis groups on one segment (they share its records in the scalar cache)
constexpr u32 RG_UNROLL = 4;   // records of one trip of k_ransac_count's loop
// (the plan -- segment_plan and its constants --: pcpx_ransac.h)
// the doubles of the fit's state: [0] the number of usable pairs, [1..3] sum p, [4..6] sum q, [8..10] pbar, [11..13] qbar,
// [16..24] H, [32] sum of squared residuals, [40..55] the transform
constexpr u32 FIT_STATE = 64, FS_N = 0, FS_SUM = 1, FS_PBAR = 8, FS_QBAR = 11, FS_H = 16, FS_SS = 32, FS_XF = 40;
constexpr size_t FIT_SCRATCH_BYTES = fit_bytes(FIT_STATE);


struct Rec {
    float v[8];  // p - o_p, q - o_q, 0, 0
};
static_assert(sizeof(Rec) == 32, "one x8 scalar load");

// Where everything lies in the scratch of a RANSAC call (byte offsets, each a multiple of 256), from the capacity and T alone.
struct Layout {
    SegmentPlan plan;
    size_t rec = 0, counts = 0, key = 0, flag = 0, place = 0, sums = 0, positions = 0, npos = 0, xf = 0, fit = 0, bytes = 0;
    Layout(u64 hypotheses, u64 capacity) : plan(segment_plan(hypotheses, capacity))
    {
        Carve c;
        rec = c.take(capacity * sizeof(Rec));
        counts = c.take(hypotheses * plan.segments * sizeof(u32));
        key = c.take(sizeof(u64));
        flag = c.take(capacity);
        place = c.take(capacity * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(capacity)) * sizeof(u32));
        positions = c.take(capacity * sizeof(u32));
        npos = c.take(sizeof(u64));
        xf = c.take(16 * sizeof(double));
        fit = c.take(FIT_SCRATCH_BYTES);
        bytes = c.bytes();
    }
};

// the two clouds and the correspondences of a call, as the kernels see them
struct Pairs {
    const float* p;
    const float* q;
    const u32* pairs;
    const u64* d_count;  // null: capacity
    u32 np, nq, capacity;
    __device__ __forceinline__ u32 count() const { return clamped_count(d_count, capacity); }
    // the six coordinates of correspondence k (k below the capacity); false when it is not usable
    __device__ __forceinline__ bool load(u32 k, float (&x)[6]) const
    {
        const uint2 st{pairs[2ull * k], pairs[2ull * k + 1]};  // (two words: the caller's array is only 4-byte aligned, include/pcpx.h)
        if (st.x >= np || st.y >= nq) return false;
        bool finite = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x[j] = p[static_cast<u64>(st.x) * 3 + j];
            x[3 + j] = q[static_cast<u64>(st.y) * 3 + j];
            finite = finite && std::isfinite(x[j]) && std::isfinite(x[3 + j]);
        }
        return finite;
    }
    // o_p and o_q: correspondence 0's points, or zeros
    __device__ __forceinline__ void origins(u32 C, float (&o)[6]) const
    {
        float x[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool ok = C != 0 && load(0, x);
#pragma unroll
        for (int j = 0; j < 6; ++j) o[j] = ok ? x[j] : 0.f;
    }
};

__device__ __forceinline__ void store_rec(Rec* at, const Rec& r)
{
    float4* out = reinterpret_cast<float4*>(at);
    out[0] = float4{r.v[0], r.v[1], r.v[2], r.v[3]};
    out[1] = float4{r.v[4], r.v[5], r.v[6], r.v[7]};
}
__device__ __forceinline__ Rec load_rec(const Rec* at)  // (a lane's own record: vector loads)
{
    const float4* in = reinterpret_cast<const float4*>(at);
    const float4 a = in[0], b = in[1];
    return Rec{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

// One thread per correspondence below the capacity: its record.  (Those at or beyond the device's count get the NaN record; nothing reads them.)
__global__ __launch_bounds__(RG_BLOCK) void k_reg_pack(Pairs in, Rec* __restrict__ rec)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= in.capacity) return;
    const u32 C = in.count();
    Rec r{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    float x[6], o[6];
    bool ok = k < C && in.load(k, x);
    if (ok) {
        in.origins(C, o);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            r.v[j] = x[j] - o[j];
            ok = ok && std::isfinite(r.v[j]);
        }
    }
    if (!ok) r = Rec{{std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    store_rec(rec + k, r);
}

struct Pose {
    float r[9], t[3];
};

struct Frame {
    float f[9];  // [u v w] as columns, row-major
    float la2, lb2, ld2, lc2;
};
// the frame of one side of a triple (pcpx_register.h, HYPOTHESIS), x0, x1, x2 three floats each
__device__ __forceinline__ Frame frame_of(const float* x0, const float* x1, const float* x2)
{
    Frame fr;
    float a[3], b[3], d[3], u[3], c[3], w[3], v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a[j] = x1[j] - x0[j];
        b[j] = x2[j] - x0[j];
        d[j] = x2[j] - x1[j];
    }
    fr.la2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    fr.lb2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    fr.ld2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float la = sqrtf(fr.la2);
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = a[j] / la;
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
    fr.lc2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    const float lc = sqrtf(fr.lc2);
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = c[j] / lc;
    v[0] = w[1] * u[2] - w[2] * u[1];
    v[1] = w[2] * u[0] - w[0] * u[2];
    v[2] = w[0] * u[1] - w[1] * u[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) fr.f[3 * j] = u[j], fr.f[3 * j + 1] = v[j], fr.f[3 * j + 2] = w[j];
    return fr;
}

__device__ __forceinline__ bool positive_finite(float x) { return x > 0.f && x < std::numeric_limits<float>::infinity(); }  // (false for a NaN)
__device__ __forceinline__ bool similar(float lp, float lq, float s2) { return lp >= s2 * lq && lq >= s2 * lp; }

// Hypothesis h of pcpx_register.h: its pose, and whether it is valid.  k_ransac_count and k_ransac_emit both get theirs from here,
// so the winner that is written out is the one that was scored, bit for bit.
__device__ __forceinline__ bool hypothesis(const Rec* __restrict__ rec, u32 C, u32 h, u32 seed, float s2, Pose& pose)
{
#pragma unroll
    for (int j = 0; j < 9; ++j) pose.r[j] = std::numeric_limits<float>::quiet_NaN();
#pragma unroll
    for (int j = 0; j < 3; ++j) pose.t[j] = std::numeric_limits<float>::quiet_NaN();
    if (C < 3) return false;
    const u32 w = fmix32(h ^ seed);
    u32 slot[3];
#pragma unroll
    for (u32 s = 0; s < 3; ++s) slot[s] = static_cast<u32>((static_cast<u64>(fmix32(w + (s + 1u) * 0x9E3779B9u)) * C) >> 32);
    const Rec x0 = load_rec(rec + slot[0]), x1 = load_rec(rec + slot[1]), x2 = load_rec(rec + slot[2]);
    const Frame fp = frame_of(x0.v, x1.v, x2.v), fq = frame_of(x0.v + 3, x1.v + 3, x2.v + 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pose.r[3 * r + c] = (fq.f[3 * r] * fp.f[3 * c] + fq.f[3 * r + 1] * fp.f[3 * c + 1]) + fq.f[3 * r + 2] * fp.f[3 * c + 2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) pose.t[r] = x0.v[3 + r] - ((pose.r[3 * r] * x0.v[0] + pose.r[3 * r + 1] * x0.v[1]) + pose.r[3 * r + 2] * x0.v[2]);
    return slot[0] != slot[1] && slot[0] != slot[2] && slot[1] != slot[2] && positive_finite(fp.la2) && positive_finite(fp.lc2) &&
           positive_finite(fq.la2) && positive_finite(fq.lc2) && similar(fp.la2, fq.la2, s2) && similar(fp.lb2, fq.lb2, s2) &&
           similar(fp.ld2, fq.ld2, s2);
}

// 12 multiplications, 14 additions and subtractions, one comparison (false for a NaN)
__device__ __forceinline__ bool inlier(const Pose& m, const Rec& x, float tau2)
{
    const float e0 = (((m.r[0] * x.v[0] + m.r[1] * x.v[1]) + m.r[2] * x.v[2]) + m.t[0]) - x.v[3];
    const float e1 = (((m.r[3] * x.v[0] + m.r[4] * x.v[1]) + m.r[5] * x.v[2]) + m.t[1]) - x.v[4];
    const float e2 = (((m.r[6] * x.v[0] + m.r[7] * x.v[1]) + m.r[8] * x.v[2]) + m.t[2]) - x.v[5];
    return (e0 * e0 + e1 * e1) + e2 * e2 <= tau2;
}

// One wavefront per (64 consecutive hypotheses from h_base on, one segment of the records).  The lane's pose is 12 registers,
// statically indexed; a record is a 32-byte scalar load, RG_UNROLL of them issued together and waited for once (the other waves of
// the SIMD cover their latency: a load written one record ahead of its arithmetic, as in k_match, hipcc sinks to the top of the
// next trip).  counts[segment * T + h] = the lane's inliers in the segment, or RG_INVALID for an
// invalid hypothesis (every segment's wave finds that out for itself: the prologue is small beside a segment).  A wave none of whose
// hypotheses is valid skips the loop.
__global__ __launch_bounds__(64 * RG_WAVES) void k_ransac_count(const Rec* __restrict__ rec, u32 capacity, const u64* __restrict__ d_count, u64 h_base, u64 T,
                                                               u32 seed, float s2, float tau2, u64 seg_rows, u32* __restrict__ counts)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 first = h_base + (static_cast<u64>(blockIdx.x) * RG_WAVES + (threadIdx.x >> 6)) * GROUP;
    if (first >= T) return;  // (wave-uniform)
    const u64 h = first + lane;
    const bool active = h < T;
    u32 C = capacity;
    if (d_count) {
        const u64 c = load_const(d_count);
        C = c < capacity ? static_cast<u32>(c) : capacity;
    }
    Pose pose;
    const bool valid = hypothesis(rec, C, static_cast<u32>(active ? h : first), seed, s2, pose);
    // (32-bit positions: the loop's bookkeeping stays on the scalar unit)
    const u64 begin = blockIdx.y * seg_rows, end = begin + seg_rows;
    const u32 t1 = end < C ? static_cast<u32>(end) : C;
    u32 t = begin < t1 ? static_cast<u32>(begin) : t1;  // (a segment at or beyond the count does nothing)
    if (!any_lane(active && valid)) t = t1;             // (a wave without a valid hypothesis idles: masking single lanes off saves nothing)
    u32 n = 0;
    for (; t1 - t >= RG_UNROLL; t += RG_UNROLL) {
        Rec x[RG_UNROLL];
#pragma unroll
        for (u32 j = 0; j < RG_UNROLL; ++j) x[j] = load_const(rec + t + j);
#pragma unroll
        for (u32 j = 0; j < RG_UNROLL; ++j) n += inlier(pose, x[j], tau2) ? 1u : 0u;
    }
    for (; t < t1; ++t) n += inlier(pose, load_const(rec + t), tau2) ? 1u : 0u;
    if (active) counts[static_cast<u64>(blockIdx.y) * T + h] = valid ? n : RG_INVALID;
}

// (k_ransac_best, the best-key reduction over the counts: pcpx_ransac.h)

__device__ __forceinline__ void store_identity(double* xf)
{
#pragma unroll
    for (int j = 0; j < 16; ++j) xf[j] = (j % 5 == 0) ? 1.0 : 0.0;
}

// One thread per correspondence below the capacity (one block at the least): every thread rebuilds the winner and flags its own
// correspondence; the first thread writes found, h, the score and the transform (xf is never null: the caller's array or scratch).
__global__ __launch_bounds__(RG_BLOCK) void k_ransac_emit(Pairs in, const Rec* __restrict__ rec, const u64* __restrict__ key, u32 seed, float s2, float tau2,
                                                         u32* __restrict__ out_found, u32* __restrict__ out_h, u32* __restrict__ out_score,
                                                         double* __restrict__ xf, uint8_t* __restrict__ flag)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    const u32 C = in.count();
    const u64 best = *key;
    const bool found = best != 0;
    const u32 h = 0xFFFFFFFFu - static_cast<u32>(best);
    Pose pose;
    hypothesis(rec, found ? C : 0u, h, seed, s2, pose);
    if (k < in.capacity) flag[k] = (found && k < C && inlier(pose, load_rec(rec + k), tau2)) ? 1 : 0;
    if (k != 0) return;
    *out_found = found ? 1u : 0u;
    if (out_h) *out_h = found ? h : 0u;
    if (out_score) *out_score = found ? static_cast<u32>(best >> 32) - 1u : 0u;
    if (!found) {
        store_identity(xf);
        return;
    }
    float o[6];
    in.origins(C, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double r0 = pose.r[3 * r], r1 = pose.r[3 * r + 1], r2 = pose.r[3 * r + 2];
        xf[4 * r] = r0, xf[4 * r + 1] = r1, xf[4 * r + 2] = r2;
        xf[4 * r + 3] = (static_cast<double>(o[3 + r]) + static_cast<double>(pose.t[r])) -
                        ((r0 * static_cast<double>(o[0]) + r1 * static_cast<double>(o[1])) + r2 * static_cast<double>(o[2]));
    }
    xf[12] = xf[13] = xf[14] = 0.0;
    xf[15] = 1.0;
}

// (IsFlagged and k_reg_compact: pcpx_ransac.h)

// ---- the rigid fit ---------------------------------------------------------------------------------------------------------------------
// the pairs of a fit: all correspondences, or those at the listed positions
struct FitSet {
    Pairs in;
    bool listed;             // false: all C correspondences; true: those at positions[0 .. items)
    const u32* positions;    // (may be null when listed with room for none)
    const u64* d_positions;  // null: positions_capacity
    u32 positions_capacity;
    __device__ __forceinline__ u32 items(u32 C) const { return listed ? clamped_count(d_positions, positions_capacity) : C; }
    __device__ __forceinline__ bool load(u32 C, u32 j, double (&x)[6]) const
    {
        const u32 k = listed ? positions[j] : j;
        float f[6];
        if (k >= C || !in.load(k, f)) return false;
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = f[i];
        return true;
    }
};

// The three sums of the fit, in pcpx_fixed_sum.h's order.  Pass 1: the number of usable pairs and the sums of their points, and from
// them the centroids.  Pass 2: H about the centroids.  Pass 3: the squared residuals under the transform, and from them the root
// mean square (NaN with fewer than three usable pairs).
template <int PASS>
struct RigidSum {
    static constexpr int TERMS = PASS == 1 ? 7 : PASS == 2 ? 9 : 1, STRIDE = FIT_TERMS;
    FitSet set;
    double* state;
    double* out_rms;  // (pass 3)
    u32 C;            // (items() leaves the number of correspondences here for add())
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ u32 items()
    {
        C = set.in.count();
        return set.items(C);
    }
    __device__ __forceinline__ void add(u32 j, double (&acc)[TERMS]) const
    {
        double x[6];
        if (!set.load(C, j, x)) return;
        if constexpr (PASS == 1) {
            acc[0] += 1.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[1 + i] += x[i];
        } else if constexpr (PASS == 2) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[3 * a + b] += (x[a] - state[FS_PBAR + a]) * (x[3 + b] - state[FS_QBAR + b]);
            }
        } else {
            const double* m = state + FS_XF;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double e = (((m[4 * r] * x[0] + m[4 * r + 1] * x[1]) + m[4 * r + 2] * x[2]) + m[4 * r + 3]) - x[3 + r];
                acc[0] += e * e;
            }
        }
    }
    __device__ __forceinline__ void finish(u32 term, double sum) const
    {
        if constexpr (PASS == 1) {
            const double n = __shfl(sum, 0);
            state[FS_N + term] = sum;  // (FS_SUM = FS_N + 1)
            if (term >= 1) state[FS_PBAR + term - 1] = n > 0.0 ? sum / n : 0.0;  // (FS_QBAR = FS_PBAR + 3)
        } else if constexpr (PASS == 2) {
            state[FS_H + term] = sum;
        } else {
            const double n = state[FS_N];
            state[FS_SS] = sum;
            *out_rms = n >= 3.0 ? std::sqrt(sum / n) : std::numeric_limits<double>::quiet_NaN();
        }
    }
};
static_assert(FS_SUM == FS_N + 1 && FS_QBAR == FS_PBAR + 3, "pass 1 writes them as one run");
// (named, not RigidSum<1>: a kernel then reads k_fixed_partial<RigidCentroids> in a profile)
struct RigidCentroids : RigidSum<1> {};
struct RigidCross : RigidSum<2> {};
struct RigidResiduals : RigidSum<3> {};

// One thread: Horn's closed form on H, t = qbar - R pbar.  With fewer than three usable pairs: `fallback` (16 doubles) or the identity.
__global__ __launch_bounds__(64) void k_fit_solve(double* __restrict__ state, const double* __restrict__ fallback, double* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    double xf[16];
    if (state[FS_N] >= 3.0) {
        double h[9], r[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = state[FS_H + i];
        horn_rotation(h, r);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xf[4 * a] = r[3 * a], xf[4 * a + 1] = r[3 * a + 1], xf[4 * a + 2] = r[3 * a + 2];
            xf[4 * a + 3] = state[FS_QBAR + a] - ((r[3 * a] * state[FS_PBAR] + r[3 * a + 1] * state[FS_PBAR + 1]) + r[3 * a + 2] * state[FS_PBAR + 2]);
        }
        xf[12] = xf[13] = xf[14] = 0.0;
        xf[15] = 1.0;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) xf[j] = fallback ? fallback[j] : ((j % 5 == 0) ? 1.0 : 0.0);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        out[j] = xf[j];
        state[FS_XF + j] = xf[j];
    }
}

// The fit, enqueued on s.  scratch: FIT_SCRATCH_BYTES.
int fit_device(const FitSet& set, char* scratch, const double* d_fallback, double* d_out, double* d_out_rms, hipStream_t s)
{
    double* partial = reinterpret_cast<double*>(scratch);
    double* state = partial + static_cast<size_t>(FIT_BLOCKS) * FIT_TERMS;
    fixed_sum(RigidCentroids{{set, state, nullptr, 0u}}, partial, s);
    fixed_sum(RigidCross{{set, state, nullptr, 0u}}, partial, s);
    k_fit_solve<<<1, 64, 0, s>>>(state, d_fallback, d_out);
    if (d_out_rms) fixed_sum(RigidResiduals{{set, state, d_out_rms, 0u}}, partial, s);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

struct RansacArgs {
    u64 hypotheses;
    u32 seed;
    float tau2, s2;
    u32 flags;
};
struct RansacOut {
    u32 *found, *h, *score, *inliers;
    u64* inlier_count;
    double *xf, *refit;
};

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.
int ransac_device(const Layout& L, char* base, const Pairs& in, const RansacArgs& a, const RansacOut& o, hipStream_t s)
{
    Rec* rec = reinterpret_cast<Rec*>(base + L.rec);
    u32* counts = reinterpret_cast<u32*>(base + L.counts);
    u64* key = reinterpret_cast<u64*>(base + L.key);
    uint8_t* flag = reinterpret_cast<uint8_t*>(base + L.flag);
    u32* place = reinterpret_cast<u32*>(base + L.place);
    u32* positions = o.inliers ? o.inliers : reinterpret_cast<u32*>(base + L.positions);
    u64* npos = o.inlier_count ? o.inlier_count : reinterpret_cast<u64*>(base + L.npos);
    double* xf = o.xf ? o.xf : reinterpret_cast<double*>(base + L.xf);
    const u64 T = a.hypotheses;
    int st;
    PCPX_HIP(hipMemsetAsync(key, 0, sizeof(u64), s));
    if (in.capacity) {
        k_reg_pack<<<blocks_of(in.capacity, RG_BLOCK), RG_BLOCK, 0, s>>>(in, rec);
        for (u64 h0 = 0; h0 < T; h0 += PLAN_LAUNCH_HYPOTHESES) {
            const u64 here = std::min(PLAN_LAUNCH_HYPOTHESES, T - h0);
            const dim3 grid(blocks_of((here + GROUP - 1) / GROUP, RG_WAVES), L.plan.segments);
            k_ransac_count<<<grid, 64 * RG_WAVES, 0, s>>>(rec, in.capacity, in.d_count, h0, T, a.seed, a.s2, a.tau2, L.plan.rows, counts);
            k_ransac_best<<<blocks_of(here, RG_BLOCK * RG_BEST_PER_THREAD), RG_BLOCK, 0, s>>>(counts, h0, h0 + here, T, L.plan.segments, key);
        }
    } else {
        PCPX_HIP(hipMemsetAsync(npos, 0, sizeof(u64), s));  // (a scan of nothing writes no total)
    }
    k_ransac_emit<<<std::max<u32>(1, blocks_of(in.capacity, RG_BLOCK)), RG_BLOCK, 0, s>>>(in, rec, key, a.seed, a.s2, a.tau2, o.found, o.h, o.score, xf, flag);
    if ((st = exclusive_scan(IsFlagged{flag}, in.capacity, reinterpret_cast<u32*>(base + L.sums), place, npos, s)) != PCPX_OK) return st;
    if (in.capacity) k_reg_compact<<<blocks_of(in.capacity, RG_BLOCK), RG_BLOCK, 0, s>>>(in.capacity, flag, place, positions);
    PCPX_HIP(hipGetLastError());
    if (a.flags & PCPX_RANSAC_REFIT) {
        return fit_device(FitSet{in, true, positions, npos, in.capacity}, base + L.fit, xf, o.refit, nullptr, s);
    }
    return PCPX_OK;
}

int check_clouds(const char* what, const void* p, u64 np, const void* q, u64 nq, const void* pairs, u64 capacity)
{
    if (np > 0xFFFFFFFFull || nq > 0xFFFFFFFFull) {
        set_error("%s: %llu and %llu points: more than 2^32 - 1 of them", what, static_cast<unsigned long long>(np), static_cast<unsigned long long>(nq));
        return PCPX_ERR_INVALID;
    }
    if (capacity >= 0xFFFFFFFFull) {
        set_error("%s: %llu correspondences: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(capacity));
        return PCPX_ERR_INVALID;
    }
    if ((!p && np) || (!q && nq) || (!pairs && capacity)) {
        set_error("%s: a NULL array with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_ransac(const char* what, u64 hypotheses, float tau2, float s2, u32 flags, const void* found, const void* refit)
{
    if (hypotheses == 0 || hypotheses >= 0xFFFFFFFFull) {
        set_error("%s: hypotheses = %llu is not in 1 .. 2^32 - 2", what, static_cast<unsigned long long>(hypotheses));
        return PCPX_ERR_INVALID;
    }
    if (!(tau2 >= 0.f)) {  // (false for a NaN)
        set_error("%s: max_distance_sq = %g is negative or not a number", what, static_cast<double>(tau2));
        return PCPX_ERR_INVALID;
    }
    if (!(s2 >= 0.f && s2 <= 1.f)) {
        set_error("%s: edge_similarity_sq = %g is not in [0, 1]", what, static_cast<double>(s2));
        return PCPX_ERR_INVALID;
    }
    if (flags & ~PCPX_RANSAC_REFIT) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~PCPX_RANSAC_REFIT);
        return PCPX_ERR_INVALID;
    }
    if (!found) {
        set_error("%s: the found word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if ((flags & PCPX_RANSAC_REFIT) && !refit) {
        set_error("%s: PCPX_RANSAC_REFIT without a refit array", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_fit(const char* what, const void* positions, u64 positions_capacity, const void* out)
{
    if (positions_capacity >= 0xFFFFFFFFull) {
        set_error("%s: %llu positions: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(positions_capacity));
        return PCPX_ERR_INVALID;
    }
    if (!positions && positions_capacity) {
        set_error("%s: a NULL array of positions with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    if (!out) {
        set_error("%s: the transform array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

// the clouds and the correspondences of a host-form call on the device, uploaded in this order
Pairs staged_pairs(HostCall& call, const float* p, u64 np, const float* q, u64 nq, const u32* pairs, u64 count)
{
    const float* d_p = call.upload(p, np * 3 * sizeof(float));
    const float* d_q = call.upload(q, nq * 3 * sizeof(float));
    const u32* d_pairs = call.upload(pairs, count * 2 * sizeof(u32));
    return Pairs{d_p, d_q, d_pairs, nullptr, static_cast<u32>(np), static_cast<u32>(nq), static_cast<u32>(count)};
}

}  // namespace

size_t fit_scratch_bytes() { return FIT_SCRATCH_BYTES; }

int fit_pairs_device(const float* d_p, u32 np, const float* d_q, u32 nq, const u32* d_pairs, u32 capacity, const u64* d_count, void* d_scratch,
                     const double* d_fallback, double* d_out, double* d_out_rms, hipStream_t s)
{
    const FitSet set{Pairs{d_p, d_q, d_pairs, d_count, np, nq, capacity}, false, nullptr, nullptr, 0u};
    return fit_device(set, static_cast<char*>(d_scratch), d_fallback, d_out, d_out_rms, s);
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_ransac_plan(uint64_t hypotheses, uint64_t pairs_capacity, uint32_t* out_segments, uint64_t* out_segment_rows, uint64_t* out_scratch_bytes)
{
    static const char* what = "pcpx_ransac_plan";
    return on_host(what, [&]() -> int {
        int st = check_clouds(what, nullptr, 0, nullptr, 0, &pairs_capacity, pairs_capacity);  // (the sizes; there are no arrays)
        if (st != PCPX_OK || (st = check_ransac(what, hypotheses, 0.f, 0.f, 0, &hypotheses, nullptr)) != PCPX_OK) return st;
        const Layout L(hypotheses, pairs_capacity);
        if (out_segments) *out_segments = L.plan.segments;
        if (out_segment_rows) *out_segment_rows = L.plan.rows;
        if (out_scratch_bytes) *out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_ransac_rigid_dev(const float* d_p, uint64_t np, const float* d_q, uint64_t nq, const uint32_t* d_pairs, uint64_t pairs_capacity,
                          const uint64_t* d_opt_count, uint64_t hypotheses, uint32_t seed, float max_distance_sq, float edge_similarity_sq,
                          uint32_t flags, int device, void* stream, uint32_t* d_out_found, uint32_t* d_opt_out_hypothesis,
                          uint32_t* d_opt_out_score, uint32_t* d_opt_out_inliers, uint64_t* d_opt_out_inlier_count,
                          double* d_opt_out_transform, double* d_opt_out_refit)
{
    static const char* what = "pcpx_ransac_rigid_dev";
    int st = check_clouds(what, d_p, np, d_q, nq, d_pairs, pairs_capacity);
    if (st != PCPX_OK || (st = check_ransac(what, hypotheses, max_distance_sq, edge_similarity_sq, flags, d_out_found, d_opt_out_refit)) != PCPX_OK) return st;
    const Layout L(hypotheses, pairs_capacity);
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        const Pairs in{d_p, d_q, d_pairs, d_opt_count, static_cast<u32>(np), static_cast<u32>(nq), static_cast<u32>(pairs_capacity)};
        return ransac_device(L, base, in, RansacArgs{hypotheses, seed, max_distance_sq, edge_similarity_sq, flags},
                             RansacOut{d_out_found, d_opt_out_hypothesis, d_opt_out_score, d_opt_out_inliers, d_opt_out_inlier_count, d_opt_out_transform,
                                       d_opt_out_refit},
                             s);
    });
}

int pcpx_ransac_rigid(const float* p, uint64_t np, const float* q, uint64_t nq, const uint32_t* pairs, uint64_t count, uint64_t hypotheses,
                      uint32_t seed, float max_distance_sq, float edge_similarity_sq, uint32_t flags, int device, uint32_t* out_found,
                      uint32_t* opt_out_hypothesis, uint32_t* opt_out_score, uint32_t* opt_out_inliers, double* opt_out_transform,
                      double* opt_out_refit)
{
    static const char* what = "pcpx_ransac_rigid";
    int st = check_clouds(what, p, np, q, nq, pairs, count);
    if (st != PCPX_OK || (st = check_ransac(what, hypotheses, max_distance_sq, edge_similarity_sq, flags, out_found, opt_out_refit)) != PCPX_OK) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const bool refit = (flags & PCPX_RANSAC_REFIT) != 0;
        const Layout L(hypotheses, count);
        const Pairs in = staged_pairs(call, p, np, q, nq, pairs, count);
        // the small outputs as one block: found, h, score, a pad, the two transforms; and the positions
        RansacSmall<16>* d = call.alloc<RansacSmall<16>>(sizeof(RansacSmall<16>));
        u32* pos = opt_out_inliers ? call.alloc<u32>(count * sizeof(u32)) : nullptr;
        char* base = call.scratch(L.bytes);
        int r;
        if ((r = call.st) != PCPX_OK ||
            (r = ransac_device(L, base, in, RansacArgs{hypotheses, seed, max_distance_sq, edge_similarity_sq, flags},
                               RansacOut{&d->found, &d->h, &d->score, pos, nullptr, d->model, refit ? d->refit : nullptr}, call.s)) != PCPX_OK)
            return r;
        return ransac_copy_out(call, d, pos, out_found, opt_out_hypothesis, opt_out_score, opt_out_inliers, opt_out_transform, refit ? opt_out_refit : nullptr);
    });
}

int pcpx_rigid_fit_dev(const float* d_p, uint64_t np, const float* d_q, uint64_t nq, const uint32_t* d_pairs, uint64_t pairs_capacity,
                       const uint64_t* d_opt_count, const uint32_t* d_opt_positions, uint64_t positions_capacity,
                       const uint64_t* d_opt_positions_count, int device, void* stream, double* d_out_transform, double* d_opt_out_rms)
{
    static const char* what = "pcpx_rigid_fit_dev";
    int st = check_clouds(what, d_p, np, d_q, nq, d_pairs, pairs_capacity);
    if (st != PCPX_OK || (st = check_fit(what, d_opt_positions, positions_capacity, d_out_transform)) != PCPX_OK) return st;
    return on_leased(device, what, stream, FIT_SCRATCH_BYTES, [&](char* base, hipStream_t s) -> int {
        const Pairs in{d_p, d_q, d_pairs, d_opt_count, static_cast<u32>(np), static_cast<u32>(nq), static_cast<u32>(pairs_capacity)};
        const FitSet set{in, d_opt_positions != nullptr, d_opt_positions, d_opt_positions ? d_opt_positions_count : nullptr, static_cast<u32>(positions_capacity)};
        return fit_device(set, base, nullptr, d_out_transform, d_opt_out_rms, s);
    });
}

int pcpx_rigid_fit(const float* p, uint64_t np, const float* q, uint64_t nq, const uint32_t* pairs, uint64_t count,
                   const uint32_t* opt_positions, uint64_t positions_count, int device, double* out_transform, double* opt_out_rms)
{
    static const char* what = "pcpx_rigid_fit";
    int st = check_clouds(what, p, np, q, nq, pairs, count);
    if (st != PCPX_OK || (st = check_fit(what, opt_positions, positions_count, out_transform)) != PCPX_OK) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        double host[17];
        const Pairs in = staged_pairs(call, p, np, q, nq, pairs, count);
        double* out = call.alloc<double>(sizeof(host));
        const u32* pos = call.upload(opt_positions, positions_count * sizeof(u32));
        char* base = call.scratch(FIT_SCRATCH_BYTES);
        // (a list of no positions is a set of no pairs, not "all correspondences")
        const FitSet set{in, opt_positions != nullptr, pos, nullptr, static_cast<u32>(positions_count)};
        int r;
        if ((r = call.st) != PCPX_OK || (r = fit_device(set, base, nullptr, out, out + 16, call.s)) != PCPX_OK ||
            (r = call.download(host, out, sizeof(host))) != PCPX_OK || (r = call.wait()) != PCPX_OK)
            return r;
        std::copy(host, host + 16, out_transform);
        if (opt_out_rms) *opt_out_rms = host[16];
        return PCPX_OK;
    });
}

}  // extern "C"
