// pcpx_planes.hip -- plane detection (include/pcpx_planes.h): a fixed number of three-point plane hypotheses,
// each scored against all records, the least-squares plane of a list of rows, and the loop that peels plane after plane on the
// device.  The hot path has the form of k_ransac_count (pcpx_register.hip): one lane per hypothesis with its plane in four
// registers, a record a wave-uniform scalar load.  No LDS, no atomics but one integer maximum per wave, nothing between workgroups:
//   k_plane_begin    the words of the call's state: the number of live records, done = 0
//   k_plane_pack     rows -> 16-byte records {x - o, row}, 32-byte ones {x - o, row, N, 0} under the normal gate, NaN-marked
//   k_plane_count    one wavefront per (64 consecutive hypotheses, one segment of the live records): one count per lane
//   k_plane_fold     (pcpx_ransac.h) a hypothesis's segment counts into one word
//   k_ransac_best    (pcpx_ransac.h) the best key
//   k_plane_decide   one thread: the winner rebuilt by the same device function, found / stop, the plane in float64
//   k_plane_flag     the inlier flag and the keep flag of every live record, the label of the inliers' rows
//   pcpx_scan.h, k_reg_compact (pcpx_ransac.h), k_plane_rows     the inliers' rows in record order
//   k_fixed_partial / k_fixed_final (pcpx_fixed_sum.h) over PlaneSum<1..3>, k_pfit_solve   the float64 sums of the plane fit in the
//                    fixed order, and the smallest eigenvector (pcpx_plane_fit.h)
//   pcpx_scan.h, k_plane_keep    the records that are not inliers, in order, into the other buffer: the next round's
// Every kernel of round r returns at once when the loop stopped in an earlier round (State::done).
#include "pcpx_device.h"
#include "pcpx_lease.h"
#include "pcpx_plane_fit.h"
#include "pcpx_planes.h"
#include "pcpx_ransac.h"
#include "pcpx_scan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>

namespace pcpx {

namespace {

constexpr u32 PL_WAVES = 4;  // waves of a k_plane_count block: four consecutive hypothesis groups on one segment (they share its records in the scalar cache)
// (the plan -- segment_plan and its constants --: pcpx_ransac.h)
// the doubles of the fit's state: [0] the number of usable rows, [1..3] the sums, [4..6] the centroid, [8..13] the scatter,
// [16] the sum of squared residuals, [20..23] the plane
constexpr u32 PF_STATE = 32, PF_N = 0, PF_SUM = 1, PF_C = 4, PF_S = 8, PF_SS = 16, PF_PLANE = 20;
constexpr size_t PFIT_SCRATCH_BYTES = fit_bytes(PF_STATE);

struct Rec16 {
    float v[4];  // x - o, the row's bits
};
struct Rec32 {
    float v[8];  // x - o, the row's bits, N, 0
};
static_assert(sizeof(Rec16) == 16 && sizeof(Rec32) == 32, "one x4 or x8 scalar load");
template <bool NORMALS>
using RecOf = std::conditional_t<NORMALS, Rec32, Rec16>;
template <bool NORMALS>
constexpr u32 unroll_of() { return NORMALS ? 4u : 8u; }  // records of one trip of k_plane_count's loop: 128 bytes of scalar loads, one wait

struct Plane {
    float n[3], m;
};
struct Gate {
    float axis[3], min_axis_cos;
    u32 on;
};

// The words of a call on the device.  done: 0, or 1 + the round that stopped the loop; every kernel of a later round reads it first
// and returns.  live[r & 1]: the number of live records of round r.  win, hyp: the round's winner for its flag and fit kernels.
struct State {
    u32 done, planes, found, pad;
    u64 live[2];
    Plane win;
    double hyp[4];
};
struct Layout {
    SegmentPlan plan;
    size_t rec[2] = {0, 0}, counts = 0, key = 0, flag = 0, keep = 0, place = 0, sums = 0, positions = 0, rowsout = 0, npos = 0, state = 0, fit = 0, bytes = 0;
    Layout(u64 hypotheses, u64 capacity, bool normals, bool peel) : plan(segment_plan(hypotheses, capacity))
    {
        Carve c;
        const u64 rec_bytes = normals ? sizeof(Rec32) : sizeof(Rec16);
        rec[0] = c.take(capacity * rec_bytes);
        rec[1] = peel ? c.take(capacity * rec_bytes) : rec[0];
        counts = c.take(hypotheses * plan.segments * sizeof(u32));
        key = c.take(sizeof(u64));
        flag = c.take(capacity);
        keep = c.take(capacity);
        place = c.take(capacity * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(capacity)) * sizeof(u32));
        positions = c.take(capacity * sizeof(u32));
        rowsout = c.take(capacity * sizeof(u32));
        npos = c.take(sizeof(u64));
        state = c.take(sizeof(State));
        fit = c.take(PFIT_SCRATCH_BYTES);
        bytes = c.bytes();
    }
};

// the cloud and the rows of a call, as the kernels see them
struct Cloud {
    const float* points;
    const float* normals;  // null unless the normal gate is on
    const u32* rows;       // null: all n rows in order
    const u64* d_count;    // null: capacity
    u32 n, capacity, origin_row;
    __device__ __forceinline__ u32 count() const { return clamped_count(d_count, capacity); }
    __device__ __forceinline__ u32 row_of(u32 k) const { return rows ? rows[k] : k; }
    // the coordinates (and under the gate the normal) of a row of points; false when it is not usable
    __device__ __forceinline__ bool load(u32 row, float (&x)[3], float (&nn)[3]) const
    {
        if (row >= n) return false;
        bool finite = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x[j] = points[static_cast<u64>(row) * 3 + j];
            nn[j] = normals ? normals[static_cast<u64>(row) * 3 + j] : 0.f;
            finite = finite && std::isfinite(x[j]) && std::isfinite(nn[j]);
        }
        return finite;
    }
    // o: the origin row's point, or zeros
    __device__ __forceinline__ void origin(u32 C, float (&o)[3]) const
    {
        float x[3] = {0.f, 0.f, 0.f}, nn[3];
        bool ok = false;
        if (origin_row != PCPX_PLANE_ORIGIN_FIRST) ok = load(origin_row, x, nn);
        else if (C != 0) ok = load(row_of(0), x, nn);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = ok ? x[j] : 0.f;
    }
};

__device__ __forceinline__ void store_rec(Rec16* at, const Rec32& r) { *reinterpret_cast<float4*>(at) = float4{r.v[0], r.v[1], r.v[2], r.v[3]}; }
__device__ __forceinline__ void store_rec(Rec32* at, const Rec32& r)
{
    float4* out = reinterpret_cast<float4*>(at);
    out[0] = float4{r.v[0], r.v[1], r.v[2], r.v[3]};
    out[1] = float4{r.v[4], r.v[5], r.v[6], r.v[7]};
}
// (a lane's own record: vector loads)
__device__ __forceinline__ Rec16 load_rec(const Rec16* at)
{
    const float4 a = *reinterpret_cast<const float4*>(at);
    return Rec16{{a.x, a.y, a.z, a.w}};
}
__device__ __forceinline__ Rec32 load_rec(const Rec32* at)
{
    const float4* in = reinterpret_cast<const float4*>(at);
    const float4 a = in[0], b = in[1];
    return Rec32{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

__global__ __launch_bounds__(64) void k_plane_begin(Cloud in, State* __restrict__ st)
{
    if (threadIdx.x != 0) return;
    st->done = st->planes = st->found = st->pad = 0u;
    st->live[0] = in.count();
    st->live[1] = 0;
    st->win = Plane{{0.f, 0.f, 0.f}, 0.f};
    st->hyp[0] = st->hyp[1] = st->hyp[2] = st->hyp[3] = 0.0;
}

// One thread per row below the capacity: its record.  (Those at or beyond the device's count get the NaN record; nothing reads them.)
template <bool NORMALS>
__global__ __launch_bounds__(RG_BLOCK) void k_plane_pack(Cloud in, RecOf<NORMALS>* __restrict__ rec)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= in.capacity) return;
    const u32 C = in.count();
    Rec32 r{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    float x[3], nn[3], o[3];
    const u32 row = k < C ? in.row_of(k) : 0u;
    bool ok = k < C && in.load(row, x, nn);
    if (ok) {
        in.origin(C, o);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            r.v[j] = x[j] - o[j];
            r.v[4 + j] = nn[j];
            ok = ok && std::isfinite(r.v[j]);
        }
    }
    if (!ok) r = Rec32{{std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    r.v[3] = __uint_as_float(row);
    store_rec(rec + k, r);
}

// Hypothesis h of pcpx_planes.h: its plane, and whether it is valid.  k_plane_count and k_plane_decide both get theirs from here, so
// the winner that is written out is the one that was scored, bit for bit.
template <class Rec>
__device__ __forceinline__ bool hypothesis(const Rec* __restrict__ rec, u32 C, u32 h, u32 seed, const Gate& g, Plane& pl)
{
    pl.n[0] = pl.n[1] = pl.n[2] = pl.m = std::numeric_limits<float>::quiet_NaN();
    if (C < 3) return false;
    const u32 w = fmix32(h ^ seed);
    u32 slot[3];
#pragma unroll
    for (u32 s = 0; s < 3; ++s) slot[s] = static_cast<u32>((static_cast<u64>(fmix32(w + (s + 1u) * 0x9E3779B9u)) * C) >> 32);
    const float4 x0 = *reinterpret_cast<const float4*>(rec + slot[0]), x1 = *reinterpret_cast<const float4*>(rec + slot[1]),
                 x2 = *reinterpret_cast<const float4*>(rec + slot[2]);
    const float a[3] = {x1.x - x0.x, x1.y - x0.y, x1.z - x0.z}, b[3] = {x2.x - x0.x, x2.y - x0.y, x2.z - x0.z};
    float c[3];
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
    const float lc2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    const float lc = sqrtf(lc2);
#pragma unroll
    for (int j = 0; j < 3; ++j) pl.n[j] = c[j] / lc;
    pl.m = (pl.n[0] * x0.x + pl.n[1] * x0.y) + pl.n[2] * x0.z;
    bool ok = slot[0] != slot[1] && slot[0] != slot[2] && slot[1] != slot[2] && lc2 > 0.f && lc2 < std::numeric_limits<float>::infinity();
    if (g.on) ok = ok && fabsf((pl.n[0] * g.axis[0] + pl.n[1] * g.axis[1]) + pl.n[2] * g.axis[2]) >= g.min_axis_cos;  // (false for a NaN)
    return ok;
}

// 3 multiplications, 2 additions, a subtraction and a comparison of a magnitude (false for a NaN); under the gate as much again
__device__ __forceinline__ bool inlier(const Plane& p, const Rec16& x, float tau, float)
{
    const float e = ((p.n[0] * x.v[0] + p.n[1] * x.v[1]) + p.n[2] * x.v[2]) - p.m;
    return fabsf(e) <= tau;
}
__device__ __forceinline__ bool inlier(const Plane& p, const Rec32& x, float tau, float cosn)
{
    const float e = ((p.n[0] * x.v[0] + p.n[1] * x.v[1]) + p.n[2] * x.v[2]) - p.m;
    const float g = (p.n[0] * x.v[4] + p.n[1] * x.v[5]) + p.n[2] * x.v[6];
    return fabsf(e) <= tau && fabsf(g) >= cosn;
}

// One wavefront per (64 consecutive hypotheses from h_base on, one segment of the live records).  The lane's plane is 4 registers,
// statically indexed; a record is a 16- or 32-byte scalar load, 128 bytes of them issued together and waited for once.
// counts[segment * T + h] = the lane's inliers in the segment, or RG_INVALID for an invalid hypothesis.  A wave none of whose
// hypotheses is valid skips the loop.  live: the number of live records, at most `capacity`.  The loop is kept from the loop
// vectoriser: its form -- two trips at once in packed arithmetic, 27 scalar moves a trip to pair the operands -- measured 7-9 %
// slower on the large calls (where two and four hypotheses per lane are measured too, and lose).
template <bool NORMALS>
__global__ __launch_bounds__(64 * PL_WAVES) void k_plane_count(const RecOf<NORMALS>* __restrict__ rec, u32 capacity, const u64* __restrict__ live,
                                                              const u32* __restrict__ done, u32 round, u64 h_base, u64 T, u32 seed, Gate gate, float tau,
                                                              float cosn, u64 seg_rows, u32* __restrict__ counts)
{
    constexpr u32 UNROLL = unroll_of<NORMALS>();
    const u32 d = load_const(done);
    if (d != 0u && d <= round) return;  // (the loop stopped in an earlier round)
    const u32 lane = threadIdx.x & 63u;
    const u64 first = h_base + (static_cast<u64>(blockIdx.x) * PL_WAVES + (threadIdx.x >> 6)) * GROUP;
    if (first >= T) return;  // (wave-uniform)
    const u64 h = first + lane;
    const bool active = h < T;
    const u64 c = load_const(live);
    const u32 C = c < capacity ? static_cast<u32>(c) : capacity;
    Plane pl;
    const bool valid = hypothesis(rec, C, static_cast<u32>(active ? h : first), seed, gate, pl);
    // (32-bit positions: the loop's bookkeeping stays on the scalar unit)
    const u64 begin = blockIdx.y * seg_rows, end = begin + seg_rows;
    const u32 t1 = end < C ? static_cast<u32>(end) : C;
    u32 t = begin < t1 ? static_cast<u32>(begin) : t1;  // (a segment at or beyond the count does nothing)
    if (!any_lane(active && valid)) t = t1;             // (a wave without a valid hypothesis idles)
    u32 n = 0;
#pragma clang loop vectorize(disable) interleave(disable)
    for (; t1 - t >= UNROLL; t += UNROLL) {
        RecOf<NORMALS> x[UNROLL];
#pragma unroll
        for (u32 j = 0; j < UNROLL; ++j) x[j] = load_const(rec + t + j);
#pragma unroll
        for (u32 j = 0; j < UNROLL; ++j) n += inlier(pl, x[j], tau, cosn) ? 1u : 0u;
    }
    for (; t < t1; ++t) n += inlier(pl, load_const(rec + t), tau, cosn) ? 1u : 0u;
    if (active) counts[static_cast<u64>(blockIdx.y) * T + h] = valid ? n : RG_INVALID;
}

// One thread.  The round's winner from the best key: found, and whether the loop stops here (nothing valid, or a score below
// min_inliers).  A single call (single = true, min_inliers = 0) writes found, h, score and the plane either way, zeros when nothing
// was found; the loop writes the score and the plane of a round that goes on to entry `round` (the arrays were zeroed).
template <bool NORMALS>
__global__ __launch_bounds__(64) void k_plane_decide(Cloud in, const RecOf<NORMALS>* __restrict__ rec, State* __restrict__ st, const u64* __restrict__ key,
                                                    u32 round, u32 seed, Gate gate, u32 min_inliers, bool single, u32* __restrict__ out_found,
                                                    u32* __restrict__ out_h, u32* __restrict__ out_score, double* __restrict__ out_plane)
{
    if (threadIdx.x != 0 || gone(&st->done, round)) return;
    const u64 live = st->live[round & 1u];
    const u32 C = live < in.capacity ? static_cast<u32>(live) : in.capacity;
    const u64 best = *key;
    const bool found = best != 0;
    const u32 h = 0xFFFFFFFFu - static_cast<u32>(best);
    const u32 score = found ? static_cast<u32>(best >> 32) - 1u : 0u;
    const bool stop = !found || score < min_inliers;
    Plane pl;
    hypothesis(rec, stop ? 0u : C, h, seed, gate, pl);
    double plane[4] = {0.0, 0.0, 0.0, 0.0};
    if (!stop) {
        float o[3];
        // (the origin is that of the records: round 0's count is the count the pack kernel saw)
        in.origin(in.count(), o);
        const double n0 = pl.n[0], n1 = pl.n[1], n2 = pl.n[2];
        plane[0] = n0, plane[1] = n1, plane[2] = n2;
        plane[3] = -(static_cast<double>(pl.m) + ((n0 * static_cast<double>(o[0]) + n1 * static_cast<double>(o[1])) + n2 * static_cast<double>(o[2])));
        st->planes = round + 1u;
    } else {
        pl = Plane{{0.f, 0.f, 0.f}, 0.f};
        st->done = round + 1u;
    }
    st->found = stop ? 0u : 1u;
    st->win = pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) st->hyp[j] = plane[j];
    if (single || !stop) {
        if (out_found) *out_found = stop ? 0u : 1u;
        if (out_h) *out_h = stop ? 0u : h;
        if (out_score) *out_score = stop ? 0u : score;
        if (out_plane) {
#pragma unroll
            for (int j = 0; j < 4; ++j) out_plane[j] = plane[j];
        }
    }
}

// One thread per record below the capacity: flag = it is an inlier of the round's winner, keep = it is live and not one; an
// inlier's row gets the round as its label.
template <bool NORMALS>
__global__ __launch_bounds__(RG_BLOCK) void k_plane_flag(const RecOf<NORMALS>* __restrict__ rec, u32 capacity, const State* __restrict__ st, u32 round,
                                                        float tau, float cosn, uint8_t* __restrict__ flag, uint8_t* __restrict__ keep,
                                                        u32* __restrict__ labels)
{
    if (gone(&st->done, round)) return;
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= capacity) return;
    const u64 live = st->live[round & 1u];
    const bool alive = k < live;
    const RecOf<NORMALS> x = load_rec(rec + k);
    const bool in = st->found != 0u && alive && inlier(st->win, x, tau, cosn);
    flag[k] = in ? 1 : 0;
    keep[k] = (alive && !in) ? 1 : 0;
    if (in && labels) labels[__float_as_uint(x.v[3])] = round;
}

// out_rows[j] = the row of the record at positions[j], j below the number of positions
template <class Rec>
__global__ __launch_bounds__(RG_BLOCK) void k_plane_rows(const Rec* __restrict__ rec, u32 capacity, const u32* __restrict__ positions,
                                                        const u64* __restrict__ npos, const u32* __restrict__ done, u32 round, u32* __restrict__ out_rows)
{
    if (gone(done, round)) return;
    const u32 j = blockIdx.x * RG_BLOCK + threadIdx.x;
    const u64 np = *npos;
    if (j >= capacity || j >= np) return;
    const u32 k = positions[j];
    if (k < capacity) out_rows[j] = __float_as_uint(rec[k].v[3]);
}

// the kept records, in order, into the next round's buffer
template <class Rec>
__global__ __launch_bounds__(RG_BLOCK) void k_plane_keep(const Rec* __restrict__ rec, u32 capacity, const uint8_t* __restrict__ keep,
                                                        const u32* __restrict__ place, const u32* __restrict__ done, u32 round, Rec* __restrict__ next)
{
    if (gone(done, round)) return;
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= capacity || !keep[k]) return;
    const u32 at = place[k];
    if (at >= capacity) return;
    const Rec32 wide = [&] {
        Rec32 w{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        const Rec r = load_rec(rec + k);
#pragma unroll
        for (u32 i = 0; i < sizeof(Rec) / 4; ++i) w.v[i] = r.v[i];
        return w;
    }();
    store_rec(next + at, wide);
}

__global__ __launch_bounds__(64) void k_plane_finish(const State* __restrict__ st, u32* __restrict__ out_count)
{
    if (threadIdx.x == 0) *out_count = st->planes;
}

// ---- the plane fit ---------------------------------------------------------------------------------------------------------------------
// the rows of a fit: all n rows, or those listed
struct FitRows {
    const float* points;
    const u32* rows;       // (may be null when listed with room for none)
    const u64* d_count;    // null: capacity
    u32 n, capacity;
    bool listed;
    __device__ __forceinline__ u32 items() const { return listed ? clamped_count(d_count, capacity) : n; }
    __device__ __forceinline__ bool load(u32 j, double (&x)[3]) const
    {
        const u32 row = listed ? rows[j] : j;
        if (row >= n) return false;
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float f = points[static_cast<u64>(row) * 3 + i];
            finite = finite && std::isfinite(f);
            x[i] = f;
        }
        return finite;
    }
};

// The three sums of the fit, in pcpx_fixed_sum.h's order.  Pass 1: the number of usable rows and the sums of their coordinates, and
// from them the centroid.  Pass 2: the scatter about the centroid.  Pass 3: the squared distances from the plane, and from them the
// root mean square (NaN with fewer than three usable rows).  A launch of a round after the loop stopped writes nothing.
template <int PASS>
struct PlaneSum {
    static constexpr int TERMS = PASS == 1 ? 4 : PASS == 2 ? 6 : 1, STRIDE = FIT_TERMS;
    FitRows set;
    const u32* done;
    u32 round;
    double* state;
    double* out_rms;  // (pass 3)
    __device__ __forceinline__ bool live() const { return !gone(done, round); }
    __device__ __forceinline__ u32 items() const { return set.items(); }
    __device__ __forceinline__ void add(u32 j, double (&acc)[TERMS]) const
    {
        double x[3];
        if (!set.load(j, x)) return;
        if constexpr (PASS == 1) {
            acc[0] += 1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[1 + i] += x[i];
        } else if constexpr (PASS == 2) {
            const double d0 = x[0] - state[PF_C], d1 = x[1] - state[PF_C + 1], d2 = x[2] - state[PF_C + 2];
            acc[0] += d0 * d0, acc[1] += d0 * d1, acc[2] += d0 * d2, acc[3] += d1 * d1, acc[4] += d1 * d2, acc[5] += d2 * d2;
        } else {
            const double* p = state + PF_PLANE;
            const double e = (p[0] * (x[0] - state[PF_C]) + p[1] * (x[1] - state[PF_C + 1])) + p[2] * (x[2] - state[PF_C + 2]);
            acc[0] += e * e;
        }
    }
    __device__ __forceinline__ void finish(u32 term, double sum) const
    {
        if constexpr (PASS == 1) {
            const double n = __shfl(sum, 0);
            state[PF_N + term] = sum;  // (PF_SUM = PF_N + 1)
            if (term >= 1) state[PF_C + term - 1] = n > 0.0 ? sum / n : 0.0;
        } else if constexpr (PASS == 2) {
            state[PF_S + term] = sum;
        } else {
            const double n = state[PF_N];
            state[PF_SS] = sum;
            *out_rms = n >= 3.0 ? std::sqrt(sum / n) : std::numeric_limits<double>::quiet_NaN();
        }
    }
};
static_assert(PF_SUM == PF_N + 1, "pass 1 writes them as one run");
// (named, not PlaneSum<1>: a kernel then reads k_fixed_partial<PlaneCentroid> in a profile)
struct PlaneCentroid : PlaneSum<1> {};
struct PlaneScatter : PlaneSum<2> {};
struct PlaneResiduals : PlaneSum<3> {};

// One thread: the normal from the scatter, d = -n . c.  hyp (optional, 4 doubles): the hypothesis of a RANSAC refit -- the normal's
// sign follows it, and it is the result with fewer than three usable rows (else zeros).
__global__ __launch_bounds__(64) void k_pfit_solve(double* __restrict__ state, const u32* __restrict__ done, u32 round, const double* __restrict__ hyp,
                                                  double* __restrict__ out)
{
    if (threadIdx.x != 0 || gone(done, round)) return;
    double plane[4];
    if (state[PF_N] >= 3.0) {
        double s[6], n[3];
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = state[PF_S + i];
        plane_normal_of_scatter(s, n);
        if (hyp && (n[0] * hyp[0] + n[1] * hyp[1]) + n[2] * hyp[2] < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
        plane[0] = n[0], plane[1] = n[1], plane[2] = n[2];
        plane[3] = -((n[0] * state[PF_C] + n[1] * state[PF_C + 1]) + n[2] * state[PF_C + 2]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) plane[j] = hyp ? hyp[j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out[j] = plane[j];
        state[PF_PLANE + j] = plane[j];
    }
}

// The fit, enqueued on s.  scratch: PFIT_SCRATCH_BYTES.
int pfit_device(const FitRows& set, char* scratch, const u32* d_done, u32 round, const double* d_hyp, double* d_out, double* d_out_rms, hipStream_t s)
{
    double* partial = reinterpret_cast<double*>(scratch);
    double* state = partial + static_cast<size_t>(FIT_BLOCKS) * FIT_TERMS;
    fixed_sum(PlaneCentroid{{set, d_done, round, state, nullptr}}, partial, s);
    fixed_sum(PlaneScatter{{set, d_done, round, state, nullptr}}, partial, s);
    k_pfit_solve<<<1, 64, 0, s>>>(state, d_done, round, d_hyp, d_out);
    if (d_out_rms) fixed_sum(PlaneResiduals{{set, d_done, round, state, d_out_rms}}, partial, s);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

struct PlaneOut {
    u32 *found, *h, *score, *inliers;
    u64* inlier_count;
    double *plane, *refit;          // a single call: 4 doubles; the loop: max_planes x 4
    u32 *labels, *nplanes, *scores;  // the loop only
};

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.  rounds = 0: the single call.
template <bool NORMALS>
int planes_device(const Layout& L, char* base, const Cloud& in, const pcpx_plane_params& a, u32 rounds, const PlaneOut& o, hipStream_t s)
{
    using Rec = RecOf<NORMALS>;
    const bool single = rounds == 0, refit = (a.flags & PCPX_PLANE_REFIT) != 0;
    Rec* rec[2] = {reinterpret_cast<Rec*>(base + L.rec[0]), reinterpret_cast<Rec*>(base + L.rec[1])};
    u32* counts = reinterpret_cast<u32*>(base + L.counts);
    u64* key = reinterpret_cast<u64*>(base + L.key);
    uint8_t* flag = reinterpret_cast<uint8_t*>(base + L.flag);
    uint8_t* keep = reinterpret_cast<uint8_t*>(base + L.keep);
    u32* place = reinterpret_cast<u32*>(base + L.place);
    u32* sums = reinterpret_cast<u32*>(base + L.sums);
    u32* positions = reinterpret_cast<u32*>(base + L.positions);
    u32* rowsout = o.inliers ? o.inliers : reinterpret_cast<u32*>(base + L.rowsout);
    u64* npos = o.inlier_count ? o.inlier_count : reinterpret_cast<u64*>(base + L.npos);
    State* st = reinterpret_cast<State*>(base + L.state);
    const Gate gate{{a.axis[0], a.axis[1], a.axis[2]}, a.min_axis_cos, (a.flags & PCPX_PLANE_AXIS) ? 1u : 0u};
    const u64 T = a.hypotheses;
    const u32 cap = in.capacity, row_blocks = blocks_of(cap, RG_BLOCK);
    int r;
    k_plane_begin<<<1, 64, 0, s>>>(in, st);
    if (!single) {
        if (in.n) PCPX_HIP(hipMemsetAsync(o.labels, 0xFF, static_cast<size_t>(in.n) * sizeof(u32), s));
        if (o.plane) PCPX_HIP(hipMemsetAsync(o.plane, 0, static_cast<size_t>(rounds) * 4 * sizeof(double), s));
        if (refit) PCPX_HIP(hipMemsetAsync(o.refit, 0, static_cast<size_t>(rounds) * 4 * sizeof(double), s));
        if (o.scores) PCPX_HIP(hipMemsetAsync(o.scores, 0, static_cast<size_t>(rounds) * sizeof(u32), s));
    }
    if (cap) k_plane_pack<NORMALS><<<row_blocks, RG_BLOCK, 0, s>>>(in, rec[0]);
    for (u32 round = 0; round < std::max(rounds, 1u); ++round) {
        const u32 cur = round & 1u;
        const u32 seed = single ? a.seed : fmix32(a.seed + round);
        PCPX_HIP(hipMemsetAsync(key, 0, sizeof(u64), s));
        if (cap) {
            for (u64 h0 = 0; h0 < T; h0 += PLAN_LAUNCH_HYPOTHESES) {
                const u64 here = std::min(PLAN_LAUNCH_HYPOTHESES, T - h0);
                const dim3 grid(blocks_of((here + GROUP - 1) / GROUP, PL_WAVES), L.plan.segments);
                k_plane_count<NORMALS><<<grid, 64 * PL_WAVES, 0, s>>>(rec[cur], cap, &st->live[cur], &st->done, round, h0, T, seed, gate, a.max_distance,
                                                                     a.min_normal_cos, L.plan.rows, counts);
                if (L.plan.segments > 1) k_plane_fold<PL_FOLD><<<blocks_of(here * PL_FOLD, RG_BLOCK), RG_BLOCK, 0, s>>>(counts, &st->done, round, h0, h0 + here, T, L.plan.segments);
                k_ransac_best<<<blocks_of(here, RG_BLOCK * RG_BEST_PER_THREAD), RG_BLOCK, 0, s>>>(counts, h0, h0 + here, T, 1u, key);
            }
        }
        k_plane_decide<NORMALS><<<1, 64, 0, s>>>(in, rec[cur], st, key, round, seed, gate, single ? 0u : a.min_inliers, single, o.found, o.h,
                                                 single ? o.score : (o.scores ? o.scores + round : nullptr),
                                                 o.plane ? o.plane + (single ? 0 : 4 * static_cast<size_t>(round)) : nullptr);
        if (cap) k_plane_flag<NORMALS><<<row_blocks, RG_BLOCK, 0, s>>>(rec[cur], cap, st, round, a.max_distance, a.min_normal_cos, flag, keep, o.labels);
        if (single || refit) {
            if (!cap) PCPX_HIP(hipMemsetAsync(npos, 0, sizeof(u64), s));  // (a scan of nothing writes no total)
            if ((r = exclusive_scan(IsFlagged{flag}, cap, sums, place, npos, s)) != PCPX_OK) return r;
            if (cap) {
                k_reg_compact<<<row_blocks, RG_BLOCK, 0, s>>>(cap, flag, place, positions);
                k_plane_rows<Rec><<<row_blocks, RG_BLOCK, 0, s>>>(rec[cur], cap, positions, npos, &st->done, round, rowsout);
            }
            if (refit) {
                const FitRows set{in.points, rowsout, npos, in.n, cap, true};
                if ((r = pfit_device(set, base + L.fit, &st->done, round, st->hyp, o.refit + (single ? 0 : 4 * static_cast<size_t>(round)), nullptr, s)) !=
                    PCPX_OK)
                    return r;
            }
        }
        if (!single && round + 1 < rounds && cap) {
            if ((r = exclusive_scan(IsFlagged{keep}, cap, sums, place, &st->live[cur ^ 1u], s)) != PCPX_OK) return r;
            k_plane_keep<Rec><<<row_blocks, RG_BLOCK, 0, s>>>(rec[cur], cap, keep, place, &st->done, round, rec[cur ^ 1u]);
        }
    }
    if (!single) k_plane_finish<<<1, 64, 0, s>>>(st, o.nplanes);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

int run_planes(const Layout& L, char* base, const Cloud& in, const pcpx_plane_params& a, u32 rounds, const PlaneOut& o, hipStream_t s)
{
    return (a.flags & PCPX_PLANE_NORMALS) ? planes_device<true>(L, base, in, a, rounds, o, s) : planes_device<false>(L, base, in, a, rounds, o, s);
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
int check_cloud(const char* what, const void* points, u64 n, const void* rows, u64 capacity)
{
    if (n >= 0xFFFFFFFFull) {
        set_error("%s: %llu points: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(n));
        return PCPX_ERR_INVALID;
    }
    if (capacity >= 0xFFFFFFFFull) {
        set_error("%s: %llu rows: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(capacity));
        return PCPX_ERR_INVALID;
    }
    if (!points && n) {
        set_error("%s: a NULL array of points with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    if (!rows && capacity) {
        set_error("%s: a NULL array of rows with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_params(const char* what, const pcpx_plane_params* a, const void* normals, u64 n)
{
    if (!a) {
        set_error("%s: params is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (a->hypotheses == 0 || a->hypotheses >= 0xFFFFFFFFull) {
        set_error("%s: hypotheses = %llu is not in 1 .. 2^32 - 2", what, static_cast<unsigned long long>(a->hypotheses));
        return PCPX_ERR_INVALID;
    }
    const u32 known = PCPX_PLANE_REFIT | PCPX_PLANE_NORMALS | PCPX_PLANE_AXIS;
    if (a->flags & ~known) {
        set_error("%s: unknown flag bits 0x%x", what, a->flags & ~known);
        return PCPX_ERR_INVALID;
    }
    if (!(a->max_distance >= 0.f)) {  // (false for a NaN)
        set_error("%s: max_distance = %g is negative or not a number", what, static_cast<double>(a->max_distance));
        return PCPX_ERR_INVALID;
    }
    if (a->flags & PCPX_PLANE_NORMALS) {
        if (!normals && n) {
            set_error("%s: PCPX_PLANE_NORMALS without normals", what);
            return PCPX_ERR_INVALID;
        }
        if (!(a->min_normal_cos >= 0.f && a->min_normal_cos <= 1.f)) {
            set_error("%s: min_normal_cos = %g is not in [0, 1]", what, static_cast<double>(a->min_normal_cos));
            return PCPX_ERR_INVALID;
        }
    }
    if (a->flags & PCPX_PLANE_AXIS) {
        if (!(a->min_axis_cos >= 0.f && a->min_axis_cos <= 1.f)) {
            set_error("%s: min_axis_cos = %g is not in [0, 1]", what, static_cast<double>(a->min_axis_cos));
            return PCPX_ERR_INVALID;
        }
        const bool finite = std::isfinite(a->axis[0]) && std::isfinite(a->axis[1]) && std::isfinite(a->axis[2]);
        if (!finite || (a->axis[0] == 0.f && a->axis[1] == 0.f && a->axis[2] == 0.f)) {
            set_error("%s: the axis (%g, %g, %g) is zero or not finite", what, static_cast<double>(a->axis[0]), static_cast<double>(a->axis[1]),
                      static_cast<double>(a->axis[2]));
            return PCPX_ERR_INVALID;
        }
    }
    return PCPX_OK;
}

int check_single(const char* what, const pcpx_plane_params* a, const void* found, const void* refit)
{
    if (!found) {
        set_error("%s: the found word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if ((a->flags & PCPX_PLANE_REFIT) && !refit) {
        set_error("%s: PCPX_PLANE_REFIT without a refit array", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_peel(const char* what, const pcpx_plane_params* a, u64 n, const void* labels, const void* count, const void* refits)
{
    if (a->max_planes == 0 || a->max_planes > PCPX_PLANES_MAX) {
        set_error("%s: max_planes = %u is not in 1 .. %u", what, a->max_planes, PCPX_PLANES_MAX);
        return PCPX_ERR_INVALID;
    }
    if (!labels && n) {
        set_error("%s: the labels array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!count) {
        set_error("%s: the count word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if ((a->flags & PCPX_PLANE_REFIT) && !refits) {
        set_error("%s: PCPX_PLANE_REFIT without a refit array", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_pfit(const char* what, const void* out)
{
    if (!out) {
        set_error("%s: the plane array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

inline const float* gate_normals(const pcpx_plane_params* a, const float* normals) { return (a->flags & PCPX_PLANE_NORMALS) ? normals : nullptr; }

}  // namespace
}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_plane_plan(uint64_t hypotheses, uint64_t rows_capacity, uint32_t flags, uint32_t max_planes, uint32_t* out_segments,
                    uint64_t* out_segment_rows, uint64_t* out_scratch_bytes)
{
    static const char* what = "pcpx_plane_plan";
    return on_host(what, [&]() -> int {
        pcpx_plane_params a{};
        a.hypotheses = hypotheses;
        a.flags = flags & PCPX_PLANE_NORMALS;
        int st = check_cloud(what, nullptr, 0, &rows_capacity, rows_capacity);  // (the sizes; there are no arrays)
        if (st != PCPX_OK || (st = check_params(what, &a, &a, 0)) != PCPX_OK) return st;
        if (flags & ~(PCPX_PLANE_REFIT | PCPX_PLANE_NORMALS | PCPX_PLANE_AXIS)) {
            set_error("%s: unknown flag bits 0x%x", what, flags & ~(PCPX_PLANE_REFIT | PCPX_PLANE_NORMALS | PCPX_PLANE_AXIS));
            return PCPX_ERR_INVALID;
        }
        if (max_planes > PCPX_PLANES_MAX) {
            set_error("%s: max_planes = %u is above %u", what, max_planes, PCPX_PLANES_MAX);
            return PCPX_ERR_INVALID;
        }
        const Layout L(hypotheses, rows_capacity, (flags & PCPX_PLANE_NORMALS) != 0, max_planes > 1);
        if (out_segments) *out_segments = L.plan.segments;
        if (out_segment_rows) *out_segment_rows = L.plan.rows;
        if (out_scratch_bytes) *out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_plane_ransac_dev(const float* d_points, uint64_t n, const float* d_opt_normals, const uint32_t* d_opt_rows, uint64_t rows_capacity,
                          const uint64_t* d_opt_rows_count, const pcpx_plane_params* params, int device, void* stream, uint32_t* d_out_found,
                          uint32_t* d_opt_out_hypothesis, uint32_t* d_opt_out_score, uint32_t* d_opt_out_inliers,
                          uint64_t* d_opt_out_inlier_count, double* d_opt_out_plane, double* d_opt_out_refit)
{
    static const char* what = "pcpx_plane_ransac_dev";
    int st = check_cloud(what, d_points, n, d_opt_rows, rows_capacity);
    if (st != PCPX_OK || (st = check_params(what, params, d_opt_normals, n)) != PCPX_OK || (st = check_single(what, params, d_out_found, d_opt_out_refit)) != PCPX_OK)
        return st;
    const u64 capacity = d_opt_rows ? rows_capacity : n;
    const Layout L(params->hypotheses, capacity, (params->flags & PCPX_PLANE_NORMALS) != 0, false);
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        const Cloud in{d_points, gate_normals(params, d_opt_normals), d_opt_rows, d_opt_rows ? d_opt_rows_count : nullptr, static_cast<u32>(n),
                       static_cast<u32>(capacity), params->origin_row};
        const PlaneOut out{d_out_found, d_opt_out_hypothesis, d_opt_out_score, d_opt_out_inliers, d_opt_out_inlier_count, d_opt_out_plane, d_opt_out_refit,
                           nullptr, nullptr, nullptr};
        return run_planes(L, base, in, *params, 0, out, s);
    });
}

int pcpx_plane_ransac(const float* points, uint64_t n, const float* opt_normals, const uint32_t* opt_rows, uint64_t rows_count,
                      const pcpx_plane_params* params, int device, uint32_t* out_found, uint32_t* opt_out_hypothesis, uint32_t* opt_out_score,
                      uint32_t* opt_out_inliers, double* opt_out_plane, double* opt_out_refit)
{
    static const char* what = "pcpx_plane_ransac";
    int st = check_cloud(what, points, n, opt_rows, rows_count);
    if (st != PCPX_OK || (st = check_params(what, params, opt_normals, n)) != PCPX_OK || (st = check_single(what, params, out_found, opt_out_refit)) != PCPX_OK)
        return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const u64 capacity = opt_rows ? rows_count : n;
        const bool gated = (params->flags & PCPX_PLANE_NORMALS) != 0, refit = (params->flags & PCPX_PLANE_REFIT) != 0;
        const Layout L(params->hypotheses, capacity, gated, false);
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const float* d_normals = call.upload(gated ? opt_normals : nullptr, n * 3 * sizeof(float));
        const u32* d_rows = call.upload(opt_rows, rows_count * sizeof(u32));
        // the small outputs as one block: found, h, score, a pad, the two planes; and the inliers' rows
        RansacSmall<4>* d = call.alloc<RansacSmall<4>>(sizeof(RansacSmall<4>));
        u32* inl = opt_out_inliers ? call.alloc<u32>(capacity * sizeof(u32)) : nullptr;
        char* base = call.scratch(L.bytes);
        // (a list of no rows is a set of no rows, not "all rows": the kernels tell the two apart by the pointer)
        if (opt_rows && !rows_count) d_rows = call.alloc<u32>(sizeof(u32));
        int r;
        if ((r = call.st) != PCPX_OK) return r;
        const Cloud cloud{d_points, d_normals, d_rows, nullptr, static_cast<u32>(n), static_cast<u32>(capacity), params->origin_row};
        const PlaneOut out{&d->found, &d->h, &d->score, inl, nullptr, d->model, refit ? d->refit : nullptr, nullptr, nullptr, nullptr};
        if ((r = run_planes(L, base, cloud, *params, 0, out, call.s)) != PCPX_OK) return r;
        return ransac_copy_out(call, d, inl, out_found, opt_out_hypothesis, opt_out_score, opt_out_inliers, opt_out_plane, refit ? opt_out_refit : nullptr);
    });
}

int pcpx_plane_fit_dev(const float* d_points, uint64_t n, const uint32_t* d_opt_rows, uint64_t rows_capacity, const uint64_t* d_opt_rows_count,
                       int device, void* stream, double* d_out_plane, double* d_opt_out_rms)
{
    static const char* what = "pcpx_plane_fit_dev";
    int st = check_cloud(what, d_points, n, d_opt_rows, rows_capacity);
    if (st != PCPX_OK || (st = check_pfit(what, d_out_plane)) != PCPX_OK) return st;
    return on_leased(device, what, stream, PFIT_SCRATCH_BYTES, [&](char* base, hipStream_t s) -> int {
        const FitRows set{d_points, d_opt_rows, d_opt_rows ? d_opt_rows_count : nullptr, static_cast<u32>(n), static_cast<u32>(rows_capacity), d_opt_rows != nullptr};
        return pfit_device(set, base, nullptr, 0, nullptr, d_out_plane, d_opt_out_rms, s);
    });
}

int pcpx_plane_fit(const float* points, uint64_t n, const uint32_t* opt_rows, uint64_t rows_count, int device, double* out_plane, double* opt_out_rms)
{
    static const char* what = "pcpx_plane_fit";
    int st = check_cloud(what, points, n, opt_rows, rows_count);
    if (st != PCPX_OK || (st = check_pfit(what, out_plane)) != PCPX_OK) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        double host[5];
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const u32* d_rows = call.upload(opt_rows, rows_count * sizeof(u32));
        double* out = call.alloc<double>(sizeof(host));
        char* base = call.scratch(PFIT_SCRATCH_BYTES);
        const FitRows set{d_points, d_rows, nullptr, static_cast<u32>(n), static_cast<u32>(rows_count), opt_rows != nullptr};
        int r;
        if ((r = call.st) != PCPX_OK || (r = pfit_device(set, base, nullptr, 0, nullptr, out, out + 4, call.s)) != PCPX_OK ||
            (r = call.download(host, out, sizeof(host))) != PCPX_OK || (r = call.wait()) != PCPX_OK)
            return r;
        std::copy(host, host + 4, out_plane);
        if (opt_out_rms) *opt_out_rms = host[4];
        return PCPX_OK;
    });
}

int pcpx_extract_planes_dev(const float* d_points, uint64_t n, const float* d_opt_normals, const pcpx_plane_params* params, int device,
                            void* stream, uint32_t* d_out_labels, uint32_t* d_out_count, double* d_opt_out_planes, double* d_opt_out_refits,
                            uint32_t* d_opt_out_scores)
{
    static const char* what = "pcpx_extract_planes_dev";
    int st = check_cloud(what, d_points, n, nullptr, 0);
    if (st != PCPX_OK || (st = check_params(what, params, d_opt_normals, n)) != PCPX_OK ||
        (st = check_peel(what, params, n, d_out_labels, d_out_count, d_opt_out_refits)) != PCPX_OK)
        return st;
    const Layout L(params->hypotheses, n, (params->flags & PCPX_PLANE_NORMALS) != 0, params->max_planes > 1);
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        const Cloud in{d_points, gate_normals(params, d_opt_normals), nullptr, nullptr, static_cast<u32>(n), static_cast<u32>(n), 0u};
        const PlaneOut out{nullptr, nullptr, nullptr, nullptr, nullptr, d_opt_out_planes, d_opt_out_refits, d_out_labels, d_out_count, d_opt_out_scores};
        return run_planes(L, base, in, *params, params->max_planes, out, s);
    });
}

int pcpx_extract_planes(const float* points, uint64_t n, const float* opt_normals, const pcpx_plane_params* params, int device,
                        uint32_t* out_labels, uint32_t* out_count, double* opt_out_planes, double* opt_out_refits, uint32_t* opt_out_scores)
{
    static const char* what = "pcpx_extract_planes";
    int st = check_cloud(what, points, n, nullptr, 0);
    if (st != PCPX_OK || (st = check_params(what, params, opt_normals, n)) != PCPX_OK ||
        (st = check_peel(what, params, n, out_labels, out_count, opt_out_refits)) != PCPX_OK)
        return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const bool gated = (params->flags & PCPX_PLANE_NORMALS) != 0, refit = (params->flags & PCPX_PLANE_REFIT) != 0;
        const u32 rounds = params->max_planes;
        const Layout L(params->hypotheses, n, gated, rounds > 1);
        // the small outputs as one block: planes, refits, scores, the count
        const size_t planes_at = 0, refits_at = static_cast<size_t>(rounds) * 4 * sizeof(double), scores_at = 2 * refits_at,
                     count_at = scores_at + static_cast<size_t>(rounds) * sizeof(u32), small_bytes = count_at + sizeof(u32);
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const float* d_normals = call.upload(gated ? opt_normals : nullptr, n * 3 * sizeof(float));
        char* d = call.alloc<char>(small_bytes);
        u32* labels = call.alloc<u32>(n * sizeof(u32));
        char* base = call.scratch(L.bytes);
        int r;
        if ((r = call.st) != PCPX_OK) return r;
        const Cloud cloud{d_points, d_normals, nullptr, nullptr, static_cast<u32>(n), static_cast<u32>(n), 0u};
        const PlaneOut out{nullptr, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<double*>(d + planes_at),
                           refit ? reinterpret_cast<double*>(d + refits_at) : nullptr, labels, reinterpret_cast<u32*>(d + count_at),
                           reinterpret_cast<u32*>(d + scores_at)};
        if ((r = run_planes(L, base, cloud, *params, rounds, out, call.s)) != PCPX_OK) return r;
        std::vector<char> host(small_bytes);
        if ((r = call.download(host.data(), d, small_bytes)) != PCPX_OK || (n && (r = call.download(out_labels, labels, n * sizeof(u32))) != PCPX_OK) ||
            (r = call.wait()) != PCPX_OK)
            return r;
        std::memcpy(out_count, host.data() + count_at, sizeof(u32));
        if (opt_out_planes) std::memcpy(opt_out_planes, host.data() + planes_at, refits_at);
        if (refit) std::memcpy(opt_out_refits, host.data() + refits_at, refits_at);
        if (opt_out_scores) std::memcpy(opt_out_scores, host.data() + scores_at, static_cast<size_t>(rounds) * sizeof(u32));
        return PCPX_OK;
    });
}

}  // extern "C"
