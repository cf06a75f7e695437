// pcpx_shapes.hip -- sphere and cylinder detection (include/pcpx_shapes.h): a fixed number of hypotheses from
// two oriented points each, every one scored against all records, and the closed-form least-squares sphere or cylinder of a list of
// rows.  The hot path has the form of k_plane_count (pcpx_planes.hip): one lane per hypothesis with its shape in registers, a record
// a wave-uniform scalar load, no square root and no division per record.  No LDS, no atomics but one integer maximum per wave:
//   k_shape_pack     rows -> two arrays of 16-byte records, {x - o, row} and {N, 0}, NaN-marked
//   k_shape_count    one wavefront per (64 consecutive hypotheses, one segment of the records): one count per lane
//   k_plane_fold, k_ransac_best    (pcpx_ransac.h) a hypothesis's segment counts into one word, the best key
//   k_shape_decide   one thread: the winner rebuilt by the same device function, found, the model in float64
//   k_shape_flag     the inlier flag of every record
//   pcpx_scan.h, k_reg_compact (pcpx_ransac.h), k_shape_rows     the inliers' rows in record order
//   k_fixed_partial / k_fixed_final (pcpx_fixed_sum.h) over ShapeSum<KIND, 1..3>, k_sfit_axis, k_sfit_solve   the float64 sums of
//                    the shape fit in the fixed order, the Jacobi axis (pcpx_plane_fit.h) and the 3 x 3 Cholesky solve
#include "pcpx_device.h"
#include "pcpx_lease.h"
#include "pcpx_plane_fit.h"
#include "pcpx_ransac.h"
#include "pcpx_scan.h"
#include "pcpx_shapes.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace pcpx {

namespace {

constexpr u32 SH_WAVES = 4;  // waves of a k_shape_count block: four consecutive hypothesis groups on one segment
// the doubles of the fit's state: [0] the number of usable rows, [1..3] the sums, [4..9] the normals' products, [10..12] m,
// [13..15] u, [16..25] the ten sums of pass 2, [26] the sum of squared residuals, [27] 1.0: degenerate, [28..35] the model
constexpr u32 SF_STATE = 40, SF_N = 0, SF_SUM = 1, SF_NN = 4, SF_M = 10, SF_U = 13, SF_S = 16, SF_SS = 26, SF_BAD = 27, SF_MODEL = 28;
constexpr size_t SFIT_SCRATCH_BYTES = fit_bytes(SF_STATE);

struct Rec16 {
    float v[4];  // x - o and the row's bits; or N and 0
};
static_assert(sizeof(Rec16) == 16, "one x4 scalar load");
template <bool NORMALS>
constexpr u32 unroll_of() { return NORMALS ? 4u : 8u; }  // records of one trip of k_shape_count's loop: 128 bytes of scalar loads, one wait

// A hypothesis: c the sphere's centre or a point of the cylinder's axis, u the axis (cylinder), R.
struct Shape {
    float c[3], u[3], R;
};
// what a lane keeps of it for the loop
struct Band {
    float lo2, hi2, cos2;
};
struct Gate {
    float axis[3], min_axis_cos, sin2, rmin, rmax;
    u32 axis_on;
};

struct State {
    u32 found, pad;
    Shape win;
    double hyp[8];
};

struct Layout {
    SegmentPlan plan;
    size_t xs = 0, ns = 0, counts = 0, key = 0, flag = 0, place = 0, sums = 0, positions = 0, rowsout = 0, npos = 0, state = 0, fit = 0, bytes = 0;
    Layout(u64 hypotheses, u64 capacity) : plan(segment_plan(hypotheses, capacity))
    {
        Carve c;
        xs = c.take(capacity * sizeof(Rec16));
        ns = c.take(capacity * sizeof(Rec16));
        counts = c.take(hypotheses * std::max<u64>(plan.segments, 1) * sizeof(u32));
        key = c.take(sizeof(u64));
        flag = c.take(capacity);
        place = c.take(capacity * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(capacity)) * sizeof(u32));
        positions = c.take(capacity * sizeof(u32));
        rowsout = c.take(capacity * sizeof(u32));
        npos = c.take(sizeof(u64));
        state = c.take(sizeof(State));
        fit = c.take(SFIT_SCRATCH_BYTES);
        bytes = c.bytes();
    }
};

// the cloud and the rows of a call, as the kernels see them
struct Cloud {
    const float* points;
    const float* normals;
    const u32* rows;     // null: all n rows in order
    const u64* d_count;  // null: capacity
    u32 n, capacity, origin_row;
    __device__ __forceinline__ u32 count() const { return clamped_count(d_count, capacity); }
    __device__ __forceinline__ u32 row_of(u32 k) const { return rows ? rows[k] : k; }
    // the coordinates and the normal of a row of points; false when it is not usable
    __device__ __forceinline__ bool load(u32 row, float (&x)[3], float (&nn)[3]) const
    {
        if (row >= n) return false;
        bool finite = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x[j] = points[static_cast<u64>(row) * 3 + j];
            nn[j] = normals[static_cast<u64>(row) * 3 + j];
            finite = finite && std::isfinite(x[j]) && std::isfinite(nn[j]);
        }
        return finite;
    }
    // o: the origin row's point, or zeros
    __device__ __forceinline__ void origin(u32 C, float (&o)[3]) const
    {
        float x[3] = {0.f, 0.f, 0.f}, nn[3];
        bool ok = false;
        if (origin_row != PCPX_SHAPE_ORIGIN_FIRST) ok = load(origin_row, x, nn);
        else if (C != 0) ok = load(row_of(0), x, nn);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = ok ? x[j] : 0.f;
    }
};

// One thread per row below the capacity: its two records.  (Those at or beyond the count get the NaN record; nothing reads them.)
__global__ __launch_bounds__(RG_BLOCK) void k_shape_pack(Cloud in, Rec16* __restrict__ xs, Rec16* __restrict__ ns)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= in.capacity) return;
    const u32 C = in.count();
    float x[3], nn[3], o[3], d[3] = {0.f, 0.f, 0.f};
    const u32 row = k < C ? in.row_of(k) : 0u;
    bool ok = k < C && in.load(row, x, nn);
    if (ok) {
        in.origin(C, o);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            d[j] = x[j] - o[j];
            ok = ok && std::isfinite(d[j]);
        }
    }
    float4 a{std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f, __uint_as_float(row)}, b{0.f, 0.f, 0.f, 0.f};
    if (ok) a.x = d[0], a.y = d[1], a.z = d[2], b.x = nn[0], b.y = nn[1], b.z = nn[2];
    *reinterpret_cast<float4*>(xs + k) = a;
    *reinterpret_cast<float4*>(ns + k) = b;
}

__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float (&p)[3], const float (&q)[3], float (&out)[3])
{
    out[0] = p[1] * q[2] - p[2] * q[1];
    out[1] = p[2] * q[0] - p[0] * q[2];
    out[2] = p[0] * q[1] - p[1] * q[0];
}

// q of pcpx_shapes.h's SCORE for the point x, and e: the sphere's e = x - c, the cylinder's the part of it across the axis
template <u32 KIND>
__device__ __forceinline__ float across(const Shape& sh, const float (&x)[3], float (&e)[3])
{
    const float d[3] = {x[0] - sh.c[0], x[1] - sh.c[1], x[2] - sh.c[2]};
    if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
        const float s = dot3(d, sh.u);
#pragma unroll
        for (int j = 0; j < 3; ++j) e[j] = d[j] - s * sh.u[j];
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) e[j] = d[j];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// Hypothesis h of pcpx_shapes.h: its shape, and whether it is valid.  k_shape_count and k_shape_decide both get theirs from here, so
// the winner that is written out is the one that was scored, bit for bit.
template <u32 KIND>
__device__ __forceinline__ bool hypothesis(const Rec16* __restrict__ xs, const Rec16* __restrict__ ns, u32 C, u32 h, u32 seed, const Gate& g, Shape& sh)
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    sh = Shape{{nan, nan, nan}, {nan, nan, nan}, nan};
    if (C < 2) return false;
    const u32 w0 = fmix32(h ^ seed);
    u32 slot[2];
#pragma unroll
    for (u32 s = 0; s < 2; ++s) slot[s] = static_cast<u32>((static_cast<u64>(fmix32(w0 + (s + 1u) * 0x9E3779B9u)) * C) >> 32);
    const float4 xa4 = *reinterpret_cast<const float4*>(xs + slot[0]), xb4 = *reinterpret_cast<const float4*>(xs + slot[1]);
    const float4 na4 = *reinterpret_cast<const float4*>(ns + slot[0]), nb4 = *reinterpret_cast<const float4*>(ns + slot[1]);
    const float xa[3] = {xa4.x, xa4.y, xa4.z}, xb[3] = {xb4.x, xb4.y, xb4.z}, na[3] = {na4.x, na4.y, na4.z}, nb[3] = {nb4.x, nb4.y, nb4.z};
    float w[3], rb[3], ra[3];
    cross3(na, nb, w);
    const float lw2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float r[3] = {xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2]};
    cross3(r, nb, rb);
    cross3(r, na, ra);
    const float s = dot3(rb, w) / lw2, t = dot3(ra, w) / lw2;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float ca = xa[j] + s * na[j], cb = xb[j] + t * nb[j];
        sh.c[j] = 0.5f * (ca + cb);
    }
    if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
        const float lw = sqrtf(lw2);
#pragma unroll
        for (int j = 0; j < 3; ++j) sh.u[j] = w[j] / lw;
    }
    float e[3];
    const float qa = across<KIND>(sh, xa, e), qb = across<KIND>(sh, xb, e);
    sh.R = 0.5f * (sqrtf(qa) + sqrtf(qb));
    const float inf = std::numeric_limits<float>::infinity();
    bool ok = slot[0] != slot[1] && lw2 > 0.f && lw2 < inf && lw2 >= g.sin2;
    ok = ok && std::isfinite(sh.c[0]) && std::isfinite(sh.c[1]) && std::isfinite(sh.c[2]) && std::isfinite(sh.R);
    ok = ok && g.rmin <= sh.R && sh.R <= g.rmax;
    if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
        if (g.axis_on) ok = ok && fabsf(dot3(sh.u, g.axis)) >= g.min_axis_cos;  // (false for a NaN)
    }
    return ok;
}

__device__ __forceinline__ Band band_of(const Shape& sh, float tau, float cosn)
{
    const float lo = fmaxf(sh.R - tau, 0.f), hi = sh.R + tau;
    return Band{lo * lo, hi * hi, cosn * cosn};
}

// sphere: 3 subtractions, 3 multiplications, 2 additions, 2 comparisons; the cylinder 6 multiplications, 2 additions and 3
// subtractions more; the gate 4 multiplications, 2 additions and a comparison.  All comparisons are false for a NaN.
template <u32 KIND, bool NORMALS>
__device__ __forceinline__ bool inlier(const Shape& sh, const Band& b, const Rec16& x, const Rec16& nn)
{
    float e[3];
    const float px[3] = {x.v[0], x.v[1], x.v[2]};
    const float q = across<KIND>(sh, px, e);
    bool in = b.lo2 <= q && q <= b.hi2;
    if constexpr (NORMALS) {
        const float g = (e[0] * nn.v[0] + e[1] * nn.v[1]) + e[2] * nn.v[2];
        in = in && g * g >= b.cos2 * q;
    }
    return in;
}

// One wavefront per (64 consecutive hypotheses from h_base on, one segment of the records).  The lane's shape is 6 to 10 registers,
// statically indexed; a record is a 16-byte scalar load (two under the normal gate), 128 bytes of them issued together and waited
// for once.  counts[segment * T + h] = the lane's inliers in the segment, or RG_INVALID for an invalid hypothesis.  A wave none of
// whose hypotheses is valid skips the loop.  The loop is kept from the loop vectoriser as k_plane_count's is.
template <u32 KIND, bool NORMALS>
__global__ __launch_bounds__(64 * SH_WAVES) void k_shape_count(const Rec16* __restrict__ xs, const Rec16* __restrict__ ns, u32 capacity,
                                                              const u64* __restrict__ d_count, u64 h_base, u64 T, u32 seed, Gate gate, float tau,
                                                              float cosn, u64 seg_rows, u32* __restrict__ counts)
{
    constexpr u32 UNROLL = unroll_of<NORMALS>();
    const u32 lane = threadIdx.x & 63u;
    const u64 first = h_base + (static_cast<u64>(blockIdx.x) * SH_WAVES + (threadIdx.x >> 6)) * GROUP;
    if (first >= T) return;  // (wave-uniform)
    const u64 h = first + lane;
    const bool active = h < T;
    u32 C = capacity;
    if (d_count) {
        const u64 c = load_const(d_count);
        C = c < capacity ? static_cast<u32>(c) : capacity;
    }
    Shape sh;
    const bool valid = hypothesis<KIND>(xs, ns, C, static_cast<u32>(active ? h : first), seed, gate, sh);
    const Band band = band_of(sh, tau, cosn);
    // (32-bit positions: the loop's bookkeeping stays on the scalar unit)
    const u64 begin = blockIdx.y * seg_rows, end = begin + seg_rows;
    const u32 t1 = end < C ? static_cast<u32>(end) : C;
    u32 t = begin < t1 ? static_cast<u32>(begin) : t1;  // (a segment at or beyond the count does nothing)
    if (!any_lane(active && valid)) t = t1;             // (a wave without a valid hypothesis idles)
    u32 n = 0;
#pragma clang loop vectorize(disable) interleave(disable)
    for (; t1 - t >= UNROLL; t += UNROLL) {
        Rec16 x[UNROLL], nn[UNROLL];
#pragma unroll
        for (u32 j = 0; j < UNROLL; ++j) {
            x[j] = load_const(xs + t + j);
            if constexpr (NORMALS) nn[j] = load_const(ns + t + j);
            else nn[j] = Rec16{{0.f, 0.f, 0.f, 0.f}};
        }
#pragma unroll
        for (u32 j = 0; j < UNROLL; ++j) n += inlier<KIND, NORMALS>(sh, band, x[j], nn[j]) ? 1u : 0u;
    }
    for (; t < t1; ++t) {
        const Rec16 x = load_const(xs + t);
        Rec16 nn{{0.f, 0.f, 0.f, 0.f}};
        if constexpr (NORMALS) nn = load_const(ns + t);
        n += inlier<KIND, NORMALS>(sh, band, x, nn) ? 1u : 0u;
    }
    if (active) counts[static_cast<u64>(blockIdx.y) * T + h] = valid ? n : RG_INVALID;
}

// One thread.  The winner from the best key: found, h, score and the model in the caller's coordinates; zeros when nothing is valid.
template <u32 KIND>
__global__ __launch_bounds__(64) void k_shape_decide(Cloud in, const Rec16* __restrict__ xs, const Rec16* __restrict__ ns, State* __restrict__ st,
                                                    const u64* __restrict__ key, u32 seed, Gate gate, u32* __restrict__ out_found, u32* __restrict__ out_h,
                                                    u32* __restrict__ out_score, double* __restrict__ out_model)
{
    if (threadIdx.x != 0) return;
    const u32 C = in.count();
    const u64 best = *key;
    const bool found = best != 0;
    const u32 h = 0xFFFFFFFFu - static_cast<u32>(best);
    const u32 score = found ? static_cast<u32>(best >> 32) - 1u : 0u;
    Shape sh;
    hypothesis<KIND>(xs, ns, found ? C : 0u, h, seed, gate, sh);
    double model[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (found) {
        float o[3];
        in.origin(C, o);
#pragma unroll
        for (int j = 0; j < 3; ++j) model[j] = static_cast<double>(sh.c[j]) + static_cast<double>(o[j]);
        if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
            // the sign: the component of largest magnitude is positive, the lowest index on ties
            float big = sh.u[0];
            if (fabsf(sh.u[1]) > fabsf(big)) big = sh.u[1];
            if (fabsf(sh.u[2]) > fabsf(big)) big = sh.u[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) model[3 + j] = static_cast<double>(big < 0.f ? -sh.u[j] : sh.u[j]);
            model[6] = static_cast<double>(sh.R);
        } else {
            model[3] = static_cast<double>(sh.R);
        }
    } else {
        sh = Shape{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f};
    }
    st->found = found ? 1u : 0u;
    st->pad = 0u;
    st->win = sh;
#pragma unroll
    for (int j = 0; j < 8; ++j) st->hyp[j] = model[j];
    if (out_found) *out_found = found ? 1u : 0u;
    if (out_h) *out_h = found ? h : 0u;
    if (out_score) *out_score = score;
    if (out_model) {
#pragma unroll
        for (int j = 0; j < 8; ++j) out_model[j] = model[j];
    }
}

// One thread per record below the capacity: flag = it is an inlier of the winner.
template <u32 KIND, bool NORMALS>
__global__ __launch_bounds__(RG_BLOCK) void k_shape_flag(const Rec16* __restrict__ xs, const Rec16* __restrict__ ns, Cloud in, const State* __restrict__ st,
                                                        float tau, float cosn, uint8_t* __restrict__ flag)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k >= in.capacity) return;
    const float4 a = *reinterpret_cast<const float4*>(xs + k), b = *reinterpret_cast<const float4*>(ns + k);
    const Shape sh = st->win;
    const bool inl = st->found != 0u && k < in.count() && inlier<KIND, NORMALS>(sh, band_of(sh, tau, cosn), Rec16{{a.x, a.y, a.z, a.w}}, Rec16{{b.x, b.y, b.z, b.w}});
    flag[k] = inl ? 1 : 0;
}

// out_rows[j] = the row of the record at positions[j], j below the number of positions
__global__ __launch_bounds__(RG_BLOCK) void k_shape_rows(const Rec16* __restrict__ xs, u32 capacity, const u32* __restrict__ positions,
                                                        const u64* __restrict__ npos, u32* __restrict__ out_rows)
{
    const u32 j = blockIdx.x * RG_BLOCK + threadIdx.x;
    const u64 np = *npos;
    if (j >= capacity || j >= np) return;
    const u32 k = positions[j];
    if (k < capacity) out_rows[j] = __float_as_uint(xs[k].v[3]);
}

// ---- the shape fit ---------------------------------------------------------------------------------------------------------------------
// the rows of a fit: all n rows, or those listed
struct FitRows {
    const float* points;
    const float* normals;  // (read by the cylinder only)
    const u32* rows;       // (may be null when listed with room for none)
    const u64* d_count;    // null: capacity
    u32 n, capacity;
    bool listed;
    __device__ __forceinline__ u32 items() const { return listed ? clamped_count(d_count, capacity) : n; }
    template <u32 KIND>
    __device__ __forceinline__ bool load(u32 j, double (&x)[3], double (&nn)[3]) const
    {
        const u32 row = listed ? rows[j] : j;
        if (row >= n) return false;
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float f = points[static_cast<u64>(row) * 3 + i];
            finite = finite && std::isfinite(f);
            x[i] = f;
            if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
                const float g = normals[static_cast<u64>(row) * 3 + i];
                finite = finite && std::isfinite(g);
                nn[i] = g;
            } else {
                nn[i] = 0.0;
            }
        }
        return finite;
    }
};

// q of the fit: y <- y - (y . u) u for the cylinder, and |y|^2
template <u32 KIND>
__device__ __forceinline__ double across64(const double* u, double (&y)[3])
{
    if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
        const double s = (y[0] * u[0] + y[1] * u[1]) + y[2] * u[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) y[j] = y[j] - s * u[j];
    }
    return (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
}

// The three sums of the fit, in pcpx_fixed_sum.h's order (pcpx_shapes.h, SHAPE FIT, steps 1, 2 and 4).
template <u32 KIND, int PASS>
struct ShapeSum {
    static constexpr int TERMS = PASS == 1 ? (KIND == PCPX_SHAPE_CYLINDER ? 10 : 4) : PASS == 2 ? 10 : 1, STRIDE = FIT_TERMS;
    FitRows set;
    double* state;
    double* out_rms;  // (pass 3)
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ u32 items() const { return set.items(); }
    __device__ __forceinline__ void add(u32 j, double (&acc)[TERMS]) const
    {
        double x[3], nn[3];
        if (!set.load<KIND>(j, x, nn)) return;
        if constexpr (PASS == 1) {
            acc[0] += 1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[1 + i] += x[i];
            if constexpr (KIND == PCPX_SHAPE_CYLINDER)
                acc[4] += nn[0] * nn[0], acc[5] += nn[0] * nn[1], acc[6] += nn[0] * nn[2], acc[7] += nn[1] * nn[1], acc[8] += nn[1] * nn[2], acc[9] += nn[2] * nn[2];
        } else if constexpr (PASS == 2) {
            double y[3] = {x[0] - state[SF_M], x[1] - state[SF_M + 1], x[2] - state[SF_M + 2]};
            const double q = across64<KIND>(state + SF_U, y);
            acc[0] += y[0] * y[0], acc[1] += y[0] * y[1], acc[2] += y[0] * y[2], acc[3] += y[1] * y[1], acc[4] += y[1] * y[2], acc[5] += y[2] * y[2];
            acc[6] += y[0] * q, acc[7] += y[1] * q, acc[8] += y[2] * q, acc[9] += q;
        } else {
            const double* m = state + SF_MODEL;
            double y[3] = {x[0] - m[0], x[1] - m[1], x[2] - m[2]};
            const double q = across64<KIND>(m + 3, y);
            const double e = std::sqrt(q) - (KIND == PCPX_SHAPE_CYLINDER ? m[6] : m[3]);
            acc[0] += e * e;
        }
    }
    __device__ __forceinline__ void finish(u32 term, double sum) const
    {
        if constexpr (PASS == 1) {
            const double n = __shfl(sum, 0);
            state[SF_N + term] = sum;  // (SF_SUM = SF_N + 1, SF_NN = SF_N + 4)
            if (term >= 1 && term <= 3) state[SF_M + term - 1] = n > 0.0 ? sum / n : 0.0;
        } else if constexpr (PASS == 2) {
            state[SF_S + term] = sum;
        } else {
            const double n = state[SF_N];
            state[SF_SS] = sum;
            *out_rms = state[SF_BAD] == 0.0 ? std::sqrt(sum / n) : std::numeric_limits<double>::quiet_NaN();
        }
    }
};
static_assert(SF_SUM == SF_N + 1 && SF_NN == SF_N + 4, "pass 1 writes them as one run");
// (named: a kernel then reads k_fixed_partial<SphereCentroid> in a profile)
struct SphereCentroid : ShapeSum<PCPX_SHAPE_SPHERE, 1> {};
struct SphereMoments : ShapeSum<PCPX_SHAPE_SPHERE, 2> {};
struct SphereResiduals : ShapeSum<PCPX_SHAPE_SPHERE, 3> {};
struct CylinderCentroid : ShapeSum<PCPX_SHAPE_CYLINDER, 1> {};
struct CylinderMoments : ShapeSum<PCPX_SHAPE_CYLINDER, 2> {};
struct CylinderResiduals : ShapeSum<PCPX_SHAPE_CYLINDER, 3> {};

// One thread: the cylinder's axis from the normals' products.
__global__ __launch_bounds__(64) void k_sfit_axis(double* __restrict__ state)
{
    if (threadIdx.x != 0) return;
    double s[6], u[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = state[SF_NN + i];
    plane_normal_of_scatter(s, u);
#pragma unroll
    for (int i = 0; i < 3; ++i) state[SF_U + i] = u[i];
}

// One thread: the Cholesky solve of step 3 and the model.  hyp (optional, 8 doubles): the hypothesis of a RANSAC refit, the result
// where the fit is degenerate (else zeros).
template <u32 KIND>
__global__ __launch_bounds__(64) void k_sfit_solve(double* __restrict__ state, const double* __restrict__ hyp, double* __restrict__ out, u32* __restrict__ out_status)
{
    if (threadIdx.x != 0) return;
    const double* S = state + SF_S;
    const double N = state[SF_N];
    double A00 = S[0], A01 = S[1], A02 = S[2], A11 = S[3], A12 = S[4], A22 = S[5];
    const double b0 = 0.5 * S[6], b1 = 0.5 * S[7], b2 = 0.5 * S[8];
    double u[3] = {0.0, 0.0, 0.0};
    if constexpr (KIND == PCPX_SHAPE_CYLINDER) {
        const double k = 0.5 * ((S[0] + S[3]) + S[5]);
#pragma unroll
        for (int i = 0; i < 3; ++i) u[i] = state[SF_U + i];
        const double k0 = k * u[0], k1 = k * u[1], k2 = k * u[2];
        A00 = A00 + k0 * u[0], A01 = A01 + k0 * u[1], A02 = A02 + k0 * u[2];
        A11 = A11 + k1 * u[1], A12 = A12 + k1 * u[2];
        A22 = A22 + k2 * u[2];
    }
    const double l00 = std::sqrt(A00), l10 = A01 / l00, l20 = A02 / l00;
    const double p1 = A11 - l10 * l10, l11 = std::sqrt(p1), l21 = (A12 - l20 * l10) / l11;
    const double p2 = A22 - (l20 * l20 + l21 * l21), l22 = std::sqrt(p2);
    const double z0 = b0 / l00, z1 = (b1 - l10 * z0) / l11, z2 = (b2 - (l20 * z0 + l21 * z1)) / l22;
    const double c2 = z2 / l22, c1 = (z1 - l21 * c2) / l11, c0 = (z0 - (l10 * c1 + l20 * c2)) / l00;
    const double R = std::sqrt(S[9] / N + ((c0 * c0 + c1 * c1) + c2 * c2));
    const bool good = N >= 4.0 && A00 > 0.0 && p1 > 0.0 && p2 > 0.0 && std::isfinite(c0) && std::isfinite(c1) && std::isfinite(c2) && std::isfinite(R);
    double model[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (good) {
        model[0] = state[SF_M] + c0, model[1] = state[SF_M + 1] + c1, model[2] = state[SF_M + 2] + c2;
        if constexpr (KIND == PCPX_SHAPE_CYLINDER) model[3] = u[0], model[4] = u[1], model[5] = u[2], model[6] = R;
        else model[3] = R;
    } else if (hyp) {
#pragma unroll
        for (int j = 0; j < 8; ++j) model[j] = hyp[j];
    }
    state[SF_BAD] = good ? 0.0 : 1.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        out[j] = model[j];
        state[SF_MODEL + j] = model[j];
    }
    if (out_status) *out_status = good ? PCPX_SHAPE_FIT_OK : PCPX_SHAPE_FIT_DEGENERATE;
}

// The fit, enqueued on s.  scratch: SFIT_SCRATCH_BYTES.
template <u32 KIND, class Sum1, class Sum2, class Sum3>
int sfit_kind(const FitRows& set, char* scratch, const double* d_hyp, double* d_out, double* d_out_rms, u32* d_out_status, hipStream_t s)
{
    double* partial = reinterpret_cast<double*>(scratch);
    double* state = partial + static_cast<size_t>(FIT_BLOCKS) * FIT_TERMS;
    fixed_sum(Sum1{{set, state, nullptr}}, partial, s);
    if (KIND == PCPX_SHAPE_CYLINDER) k_sfit_axis<<<1, 64, 0, s>>>(state);
    fixed_sum(Sum2{{set, state, nullptr}}, partial, s);
    k_sfit_solve<KIND><<<1, 64, 0, s>>>(state, d_hyp, d_out, d_out_status);
    if (d_out_rms) fixed_sum(Sum3{{set, state, d_out_rms}}, partial, s);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}
int sfit_device(u32 kind, const FitRows& set, char* scratch, const double* d_hyp, double* d_out, double* d_out_rms, u32* d_out_status, hipStream_t s)
{
    return kind == PCPX_SHAPE_CYLINDER
               ? sfit_kind<PCPX_SHAPE_CYLINDER, CylinderCentroid, CylinderMoments, CylinderResiduals>(set, scratch, d_hyp, d_out, d_out_rms, d_out_status, s)
               : sfit_kind<PCPX_SHAPE_SPHERE, SphereCentroid, SphereMoments, SphereResiduals>(set, scratch, d_hyp, d_out, d_out_rms, d_out_status, s);
}

struct ShapeOut {
    u32 *found, *h, *score, *inliers;
    u64* inlier_count;
    double *model, *refit;
};

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.
template <u32 KIND, bool NORMALS>
int shapes_device(const Layout& L, char* base, const Cloud& in, const pcpx_shape_params& a, const ShapeOut& o, hipStream_t s)
{
    const bool refit = (a.flags & PCPX_SHAPE_REFIT) != 0;
    Rec16* xs = reinterpret_cast<Rec16*>(base + L.xs);
    Rec16* ns = reinterpret_cast<Rec16*>(base + L.ns);
    u32* counts = reinterpret_cast<u32*>(base + L.counts);
    u64* key = reinterpret_cast<u64*>(base + L.key);
    uint8_t* flag = reinterpret_cast<uint8_t*>(base + L.flag);
    u32* place = reinterpret_cast<u32*>(base + L.place);
    u32* sums = reinterpret_cast<u32*>(base + L.sums);
    u32* positions = reinterpret_cast<u32*>(base + L.positions);
    u32* rowsout = o.inliers ? o.inliers : reinterpret_cast<u32*>(base + L.rowsout);
    u64* npos = o.inlier_count ? o.inlier_count : reinterpret_cast<u64*>(base + L.npos);
    State* st = reinterpret_cast<State*>(base + L.state);
    const Gate gate{{a.axis[0], a.axis[1], a.axis[2]}, a.min_axis_cos, a.min_normal_sin * a.min_normal_sin, a.min_radius, a.max_radius,
                    (a.flags & PCPX_SHAPE_AXIS) ? 1u : 0u};
    const float cosn = NORMALS ? a.min_normal_cos : 0.f;
    const u64 T = a.hypotheses;
    const u32 cap = in.capacity, row_blocks = blocks_of(cap, RG_BLOCK);
    int r;
    PCPX_HIP(hipMemsetAsync(key, 0, sizeof(u64), s));
    if (cap) {
        k_shape_pack<<<row_blocks, RG_BLOCK, 0, s>>>(in, xs, ns);
        for (u64 h0 = 0; h0 < T; h0 += PLAN_LAUNCH_HYPOTHESES) {
            const u64 here = std::min(PLAN_LAUNCH_HYPOTHESES, T - h0);
            const dim3 grid(blocks_of((here + GROUP - 1) / GROUP, SH_WAVES), L.plan.segments);
            k_shape_count<KIND, NORMALS><<<grid, 64 * SH_WAVES, 0, s>>>(xs, ns, cap, in.d_count, h0, T, a.seed, gate, a.max_distance, cosn, L.plan.rows, counts);
            if (L.plan.segments > 1) k_plane_fold<PL_FOLD><<<blocks_of(here * PL_FOLD, RG_BLOCK), RG_BLOCK, 0, s>>>(counts, nullptr, 0u, h0, h0 + here, T, L.plan.segments);
            k_ransac_best<<<blocks_of(here, RG_BLOCK * RG_BEST_PER_THREAD), RG_BLOCK, 0, s>>>(counts, h0, h0 + here, T, 1u, key);
        }
    }
    k_shape_decide<KIND><<<1, 64, 0, s>>>(in, xs, ns, st, key, a.seed, gate, o.found, o.h, o.score, o.model);
    if (cap) k_shape_flag<KIND, NORMALS><<<row_blocks, RG_BLOCK, 0, s>>>(xs, ns, in, st, a.max_distance, cosn, flag);
    if (!cap) PCPX_HIP(hipMemsetAsync(npos, 0, sizeof(u64), s));  // (a scan of nothing writes no total)
    if ((r = exclusive_scan(IsFlagged{flag}, cap, sums, place, npos, s)) != PCPX_OK) return r;
    if (cap) {
        k_reg_compact<<<row_blocks, RG_BLOCK, 0, s>>>(cap, flag, place, positions);
        k_shape_rows<<<row_blocks, RG_BLOCK, 0, s>>>(xs, cap, positions, npos, rowsout);
    }
    if (refit) {
        const FitRows set{in.points, in.normals, rowsout, npos, in.n, cap, true};
        if ((r = sfit_device(KIND, set, base + L.fit, st->hyp, o.refit, nullptr, nullptr, s)) != PCPX_OK) return r;
    }
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

int run_shapes(const Layout& L, char* base, const Cloud& in, const pcpx_shape_params& a, const ShapeOut& o, hipStream_t s)
{
    const bool gated = (a.flags & PCPX_SHAPE_NORMALS) != 0;
    if (a.kind == PCPX_SHAPE_CYLINDER)
        return gated ? shapes_device<PCPX_SHAPE_CYLINDER, true>(L, base, in, a, o, s) : shapes_device<PCPX_SHAPE_CYLINDER, false>(L, base, in, a, o, s);
    return gated ? shapes_device<PCPX_SHAPE_SPHERE, true>(L, base, in, a, o, s) : shapes_device<PCPX_SHAPE_SPHERE, false>(L, base, in, a, o, s);
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
int check_cloud(const char* what, const void* points, u64 n, const void* rows, u64 capacity, const void* count)
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
    if (!rows && (capacity || count)) {
        set_error("%s: a NULL array of rows with a non-zero size or a count", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

bool in_unit(float v) { return v >= 0.f && v <= 1.f; }  // (false for a NaN)

int check_params(const char* what, const pcpx_shape_params* a, const void* normals, u64 n, const void* stream)
{
    if (!a) {
        set_error("%s: params is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (a->kind != PCPX_SHAPE_SPHERE && a->kind != PCPX_SHAPE_CYLINDER) {
        set_error("%s: kind = %u is neither PCPX_SHAPE_SPHERE nor PCPX_SHAPE_CYLINDER", what, a->kind);
        return PCPX_ERR_INVALID;
    }
    const u32 known = PCPX_SHAPE_REFIT | PCPX_SHAPE_NORMALS | PCPX_SHAPE_AXIS | PCPX_SHAPE_ON_DEVICE;
    if (a->flags & ~known) {
        set_error("%s: unknown flag bits 0x%x", what, a->flags & ~known);
        return PCPX_ERR_INVALID;
    }
    if (a->reserved != 0u) {
        set_error("%s: reserved = %u is not 0", what, a->reserved);
        return PCPX_ERR_INVALID;
    }
    if ((a->flags & PCPX_SHAPE_AXIS) && a->kind == PCPX_SHAPE_SPHERE) {
        set_error("%s: PCPX_SHAPE_AXIS with a sphere", what);
        return PCPX_ERR_INVALID;
    }
    if (a->hypotheses == 0 || a->hypotheses >= 0xFFFFFFFFull) {
        set_error("%s: hypotheses = %llu is not in 1 .. 2^32 - 2", what, static_cast<unsigned long long>(a->hypotheses));
        return PCPX_ERR_INVALID;
    }
    if (!normals && n) {
        set_error("%s: a NULL array of normals with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    if (!(a->max_distance >= 0.f)) {  // (false for a NaN)
        set_error("%s: max_distance = %g is negative or not a number", what, static_cast<double>(a->max_distance));
        return PCPX_ERR_INVALID;
    }
    if (!(a->min_radius >= 0.f) || !(a->max_radius >= a->min_radius)) {
        set_error("%s: the radius range [%g, %g] is negative, empty or not a number", what, static_cast<double>(a->min_radius),
                  static_cast<double>(a->max_radius));
        return PCPX_ERR_INVALID;
    }
    if (!in_unit(a->min_normal_sin) || !in_unit(a->min_normal_cos) || !in_unit(a->min_axis_cos)) {
        set_error("%s: min_normal_sin = %g, min_normal_cos = %g or min_axis_cos = %g is not in [0, 1]", what, static_cast<double>(a->min_normal_sin),
                  static_cast<double>(a->min_normal_cos), static_cast<double>(a->min_axis_cos));
        return PCPX_ERR_INVALID;
    }
    if (a->flags & PCPX_SHAPE_AXIS) {
        const bool finite = std::isfinite(a->axis[0]) && std::isfinite(a->axis[1]) && std::isfinite(a->axis[2]);
        if (!finite || (a->axis[0] == 0.f && a->axis[1] == 0.f && a->axis[2] == 0.f)) {
            set_error("%s: the axis (%g, %g, %g) is zero or not finite", what, static_cast<double>(a->axis[0]), static_cast<double>(a->axis[1]),
                      static_cast<double>(a->axis[2]));
            return PCPX_ERR_INVALID;
        }
    }
    if (stream && !(a->flags & PCPX_SHAPE_ON_DEVICE)) {
        set_error("%s: a stream without PCPX_SHAPE_ON_DEVICE", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_single(const char* what, const pcpx_shape_params* a, const void* found, const void* refit)
{
    if (!found) {
        set_error("%s: the found word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if ((a->flags & PCPX_SHAPE_REFIT) && !refit) {
        set_error("%s: PCPX_SHAPE_REFIT without a refit array", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_sfit(const char* what, u32 kind, u32 flags, const void* normals, u64 n, const void* stream, const void* out)
{
    if (kind != PCPX_SHAPE_SPHERE && kind != PCPX_SHAPE_CYLINDER) {
        set_error("%s: kind = %u is neither PCPX_SHAPE_SPHERE nor PCPX_SHAPE_CYLINDER", what, kind);
        return PCPX_ERR_INVALID;
    }
    if (flags & ~PCPX_SHAPE_ON_DEVICE) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~PCPX_SHAPE_ON_DEVICE);
        return PCPX_ERR_INVALID;
    }
    if (kind == PCPX_SHAPE_CYLINDER && !normals && n) {
        set_error("%s: a cylinder without normals", what);
        return PCPX_ERR_INVALID;
    }
    if (stream && !(flags & PCPX_SHAPE_ON_DEVICE)) {
        set_error("%s: a stream without PCPX_SHAPE_ON_DEVICE", what);
        return PCPX_ERR_INVALID;
    }
    if (!out) {
        set_error("%s: the model array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_shape_plan(uint64_t hypotheses, uint64_t rows_capacity, uint32_t* out_segments, uint64_t* out_segment_rows, uint64_t* out_scratch_bytes)
{
    static const char* what = "pcpx_shape_plan";
    return on_host(what, [&]() -> int {
        const int st = check_cloud(what, nullptr, 0, &rows_capacity, rows_capacity, nullptr);  // (the sizes; there are no arrays)
        if (st != PCPX_OK) return st;
        if (hypotheses == 0 || hypotheses >= 0xFFFFFFFFull) {
            set_error("%s: hypotheses = %llu is not in 1 .. 2^32 - 2", what, static_cast<unsigned long long>(hypotheses));
            return PCPX_ERR_INVALID;
        }
        const Layout L(hypotheses, rows_capacity);
        if (out_segments) *out_segments = L.plan.segments;
        if (out_segment_rows) *out_segment_rows = L.plan.rows;
        if (out_scratch_bytes) *out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_shape_ransac(const float* points, uint64_t n, const float* normals, const uint32_t* opt_rows, uint64_t rows_capacity,
                      const uint64_t* opt_rows_count, const pcpx_shape_params* params, int device, void* stream, uint32_t* out_found,
                      uint32_t* opt_out_hypothesis, uint32_t* opt_out_score, uint32_t* opt_out_inliers, uint64_t* opt_out_inlier_count,
                      double* opt_out_model, double* opt_out_refit)
{
    static const char* what = "pcpx_shape_ransac";
    int st = check_cloud(what, points, n, opt_rows, rows_capacity, opt_rows_count);
    if (st != PCPX_OK || (st = check_params(what, params, normals, n, stream)) != PCPX_OK ||
        (st = check_single(what, params, out_found, opt_out_refit)) != PCPX_OK)
        return st;
    const bool refit = (params->flags & PCPX_SHAPE_REFIT) != 0;
    if (params->flags & PCPX_SHAPE_ON_DEVICE) {
        const u64 capacity = opt_rows ? rows_capacity : n;
        const Layout L(params->hypotheses, capacity);
        return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
            const Cloud in{points, normals, opt_rows, opt_rows ? opt_rows_count : nullptr, static_cast<u32>(n), static_cast<u32>(capacity), params->origin_row};
            const ShapeOut out{out_found, opt_out_hypothesis, opt_out_score, opt_out_inliers, opt_out_inlier_count, opt_out_model, refit ? opt_out_refit : nullptr};
            return run_shapes(L, base, in, *params, out, s);
        });
    }
    // (the host's count is read here: the call is laid out for the rows it names)
    const u64 rows_count = opt_rows_count ? std::min<u64>(*opt_rows_count, rows_capacity) : rows_capacity;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const u64 capacity = opt_rows ? rows_count : n;
        const Layout L(params->hypotheses, capacity);
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const float* d_normals = call.upload(normals, n * 3 * sizeof(float));
        const u32* d_rows = call.upload(opt_rows, rows_count * sizeof(u32));
        // the small outputs as one block: found, h, score, a pad, the two models; and the inliers' rows
        RansacSmall<8>* d = call.alloc<RansacSmall<8>>(sizeof(RansacSmall<8>));
        u32* inl = opt_out_inliers ? call.alloc<u32>(capacity * sizeof(u32)) : nullptr;
        char* base = call.scratch(L.bytes);
        // (a list of no rows is a set of no rows, not "all rows": the kernels tell the two apart by the pointer)
        if (opt_rows && !rows_count) d_rows = call.alloc<u32>(sizeof(u32));
        int r;
        if ((r = call.st) != PCPX_OK) return r;
        const Cloud cloud{d_points, d_normals, d_rows, nullptr, static_cast<u32>(n), static_cast<u32>(capacity), params->origin_row};
        const ShapeOut out{&d->found, &d->h, &d->score, inl, nullptr, d->model, refit ? d->refit : nullptr};
        if ((r = run_shapes(L, base, cloud, *params, out, call.s)) != PCPX_OK) return r;
        u32 score = 0;
        if ((r = ransac_copy_out(call, d, inl, out_found, opt_out_hypothesis, &score, opt_out_inliers, opt_out_model, refit ? opt_out_refit : nullptr)) != PCPX_OK)
            return r;
        if (opt_out_score) *opt_out_score = score;
        if (opt_out_inlier_count) *opt_out_inlier_count = score;
        return PCPX_OK;
    });
}

int pcpx_shape_fit(const float* points, uint64_t n, const float* opt_normals, const uint32_t* opt_rows, uint64_t rows_capacity,
                   const uint64_t* opt_rows_count, uint32_t kind, uint32_t flags, int device, void* stream, double* out_model, double* opt_out_rms,
                   uint32_t* opt_out_status)
{
    static const char* what = "pcpx_shape_fit";
    int st = check_cloud(what, points, n, opt_rows, rows_capacity, opt_rows_count);
    if (st != PCPX_OK || (st = check_sfit(what, kind, flags, opt_normals, n, stream, out_model)) != PCPX_OK) return st;
    if (flags & PCPX_SHAPE_ON_DEVICE)
        return on_leased(device, what, stream, SFIT_SCRATCH_BYTES, [&](char* base, hipStream_t s) -> int {
            const FitRows set{points, opt_normals, opt_rows, opt_rows ? opt_rows_count : nullptr, static_cast<u32>(n), static_cast<u32>(rows_capacity), opt_rows != nullptr};
            return sfit_device(kind, set, base, nullptr, out_model, opt_out_rms, opt_out_status, s);
        });
    const u64 rows_count = opt_rows_count ? std::min<u64>(*opt_rows_count, rows_capacity) : rows_capacity;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        struct Small {
            double model[8], rms;
            u32 status, pad;
        } host;
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const float* d_normals = call.upload(kind == PCPX_SHAPE_CYLINDER ? opt_normals : nullptr, n * 3 * sizeof(float));
        const u32* d_rows = call.upload(opt_rows, rows_count * sizeof(u32));
        Small* d = call.alloc<Small>(sizeof(Small));
        char* base = call.scratch(SFIT_SCRATCH_BYTES);
        const FitRows set{d_points, d_normals, d_rows, nullptr, static_cast<u32>(n), static_cast<u32>(rows_count), opt_rows != nullptr};
        int r;
        if ((r = call.st) != PCPX_OK || (r = sfit_device(kind, set, base, nullptr, d->model, &d->rms, &d->status, call.s)) != PCPX_OK ||
            (r = call.download(&host, d, sizeof(host))) != PCPX_OK || (r = call.wait()) != PCPX_OK)
            return r;
        std::copy(host.model, host.model + 8, out_model);
        if (opt_out_rms) *opt_out_rms = host.rms;
        if (opt_out_status) *opt_out_status = host.status;
        return PCPX_OK;
    });
}

}  // extern "C"
