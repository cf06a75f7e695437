// pcpx_mls.hip -- moving least squares projection (include/pcpx_mls.h) for gfx950: the fixed-radius moments
// walk of pcpx_range.hip with a Gaussian weight per neighbour (k_mls_plane), and for order 2 a second walk of the same sphere that
// accumulates a 6 x 6 least-squares system per lane, solved in float64 in the epilogue (k_mls_poly).  One lane = one sphere,
// lane-per-range leaves, no LDS.  Between the two kernels a lane passes one 16-byte record per position: (n, t).
#include "pcpx_stage.h"
#include "pcpx_device.h"
#include "pcpx_eig3.h"
#include "pcpx_mls.h"

#include <limits>

namespace pcpx {

namespace {

struct MlsOut {
    float* points = nullptr;     // rows x 3
    float* disp = nullptr;       // rows x 3
    float* normals = nullptr;    // rows x 3
    float* curvatures = nullptr; // rows x 2: H, K
    u32* count = nullptr;        // rows
    u32* fit = nullptr;          // rows
    bool none() const { return !points && !disp && !normals && !curvatures && !count && !fit; }
};

// What a row without a fit gets (count < 3): the centre's own bits, no displacement, the solver's normal of a zero matrix
__device__ __forceinline__ void write_unchanged(const MlsOut& out, const u64 row, const float qx, const float qy, const float qz, const u32 cnt)
{
    const u64 r3 = 3ull * row;
    if (out.points) {
        out.points[r3] = qx;
        out.points[r3 + 1] = qy;
        out.points[r3 + 2] = qz;
    }
    if (out.disp) {
        out.disp[r3] = 0.f;
        out.disp[r3 + 1] = 0.f;
        out.disp[r3 + 2] = 0.f;
    }
    if (out.normals) {
        float nrm[3], ev[3];
        eig3_smallest(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, nrm, ev);
        out.normals[r3] = nrm[0];
        out.normals[r3 + 1] = nrm[1];
        out.normals[r3 + 2] = nrm[2];
    }
    if (out.curvatures) {
        out.curvatures[2 * row] = __builtin_nanf("");
        out.curvatures[2 * row + 1] = __builtin_nanf("");
    }
    if (out.count) out.count[row] = cnt;
    if (out.fit) out.fit[row] = 0u;
}

// The lane's sphere, as range_group (pcpx_range.hip): the centre, its output row, r, r^2 (-1: an idle lane) and the weight's
// k = -1 / (h h) with h = gauss_h, or gauss_h * r / radius with one radius per sphere (a sphere of radius 0 then holds copies of its
// centre only: k = 0, weight 1)
struct MlsLane {
    float qx, qy, qz, r, r2, k;
    u32 row, p;
    bool valid;
};
template <bool SELF>
__device__ __forceinline__ MlsLane mls_lane(const TreeView& t, const QueryView& qv, const u32 g, const u32 lane, const float radius,
                                            const float* __restrict__ radii, const float gauss_h)
{
    MlsLane m;
    m.p = g * GROUP + lane;
    const u32 nq = SELF ? t.n : qv.nq;
    m.valid = m.p < nq && (!SELF || m.p - qv.pos_lo < qv.pos_hi - qv.pos_lo);  // (self ranges: only the asked positions)
    LaneQuery q{0.f, 0.f, 0.f, 0u};
    if (m.valid) q = lane_query<SELF>(t, qv, m.p);
    m.qx = q.x;
    m.qy = q.y;
    m.qz = q.z;
    m.row = q.row;
    m.r = radius;
    float h = gauss_h;
    if (radii && m.valid) {
        m.r = radii[m.row];
        h = gauss_h * m.r / radius;
    }
    m.r2 = m.valid ? m.r * m.r : -1.f;
    m.k = h > 0.f ? -1.f / (h * h) : 0.f;
    return m;
}

// Stage 1: count, W = sum w, S = sum w d, Q = sum w d d^T about the centre; the plane through m = S / W with the normal of
// C = Q - S m^T.  rec (order 2 only): (n, t) at the lane's position, n = 0 where stage 2 has nothing to do.
template <bool SELF>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_mls_plane(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                                   const float* __restrict__ radii, float gauss_h, float4* __restrict__ rec,
                                                                   MlsOut out)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const MlsLane m = mls_lane<SELF>(t, qv, g, lane, radius, radii, gauss_h);
    const float qx = m.qx, qy = m.qy, qz = m.qz, r2 = m.r2, k = m.k;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    u32 cnt = 0;
    float wsum = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, q00 = 0.f, q10 = 0.f, q11 = 0.f, q20 = 0.f, q21 = 0.f, q22 = 0.f;
    walk_needed_leaves<false>(t, need, [&](const u32, const Leaf* record, const u64, const u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const float d2 = sq3(dx, dy, dz);
            if (d2 <= r2) {  // (a NaN padding point fails)
                const float w = expf(d2 * k);
                const float wx = w * dx, wy = w * dy, wz = w * dz;
                cnt += 1u;
                wsum += w;
                s0 += wx; s1 += wy; s2 += wz;
                q00 += wx * dx; q10 += wy * dx; q11 += wy * dy;
                q20 += wz * dx; q21 += wz * dy; q22 += wz * dz;
            }
        }
    });
    if (!m.valid) return;
    const u64 row = m.row;
    if (cnt < 3u || !(wsum > 0.f)) {  // (every weight underflowed: as too few points)
        write_unchanged(out, row, qx, qy, qz, cnt);
        if (rec) rec[m.p] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float m0 = s0 / wsum, m1 = s1 / wsum, m2 = s2 / wsum;
    const float c00 = q00 - s0 * m0, c10 = q10 - s1 * m0, c11 = q11 - s1 * m1;
    const float c20 = q20 - s2 * m0, c21 = q21 - s2 * m1, c22 = q22 - s2 * m2;
    float nrm[3], ev[3];
    eig3_smallest(c00, c10, c20, c11, c21, c22, nrm, ev);
    // copies of one point (C = 0): no surface, the centre stays
    const bool flat = c00 == 0.f && c10 == 0.f && c11 == 0.f && c20 == 0.f && c21 == 0.f && c22 == 0.f;
    const float tt = flat ? 0.f : (m0 * nrm[0] + m1 * nrm[1]) + m2 * nrm[2];
    const float d0 = tt * nrm[0], d1 = tt * nrm[1], d2 = tt * nrm[2];
    const u64 r3 = 3ull * row;
    if (out.points) {
        out.points[r3] = qx + d0;
        out.points[r3 + 1] = qy + d1;
        out.points[r3 + 2] = qz + d2;
    }
    if (out.disp) {
        out.disp[r3] = d0;
        out.disp[r3 + 1] = d1;
        out.disp[r3 + 2] = d2;
    }
    if (out.normals) {
        out.normals[r3] = nrm[0];
        out.normals[r3 + 1] = nrm[1];
        out.normals[r3 + 2] = nrm[2];
    }
    if (out.curvatures) {
        out.curvatures[2 * row] = __builtin_nanf("");
        out.curvatures[2 * row + 1] = __builtin_nanf("");
    }
    if (out.count) out.count[row] = cnt;
    if (out.fit) out.fit[row] = 1u;
    if (rec) rec[m.p] = (flat || cnt < 6u) ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(nrm[0], nrm[1], nrm[2], tt);
}

// The 6 x 6 normal equations by Cholesky in float64, in the shape of plane_cholesky (pcpx_plane_solve.h) with this contract's pivot
// rule: a: the upper triangle row by row, b: the right-hand side.  false when a pivot is not finite or <= PCPX_MLS_PIVOT_MIN times
// its own diagonal entry (x is then not written).
constexpr int mls_at(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }
__device__ __forceinline__ bool mls_cholesky(const double (&a)[21], const double (&b)[6], double (&x)[6])
{
    double l[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = a[mls_at(j, j)];
#pragma unroll
        for (int i = 0; i < j; ++i) d -= l[j][i] * l[j][i];
        ok = ok && d > PCPX_MLS_PIVOT_MIN * a[mls_at(j, j)] && d < std::numeric_limits<double>::infinity();  // (false for a NaN pivot)
        const double root = sqrt(d);
        l[j][j] = root;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = a[mls_at(j, i)];
#pragma unroll
            for (int c = 0; c < j; ++c) v -= l[i][c] * l[j][c];
            l[i][j] = v / root;
        }
    }
    if (!ok) return false;
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
#pragma unroll
        for (int c = 0; c < i; ++c) v -= l[i][c] * z[c];
        z[i] = v / l[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int c = i + 1; c < 6; ++c) v -= l[c][i] * x[c];
        x[i] = v / l[i][i];
    }
    return true;
}

// Stage 2: the same sphere and weights in the frame (U, V, n) at the origin o = t n; heights z over (u, v), all divided by r (times
// the float32 reciprocal of r).  The basis b = (1, u, v, u^2, u v, v^2): the 21 unique terms of sum w b b^T are 15 different sums --
// the weighted monomials u^i v^j, i + j <= 4 -- so 15 accumulators and the 6 of sum w z b.  A row whose fit is refused keeps what
// k_mls_plane wrote.
template <bool SELF>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_mls_poly(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                                  const float* __restrict__ radii, float gauss_h,
                                                                  const float4* __restrict__ rec, MlsOut out)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    MlsLane m = mls_lane<SELF>(t, qv, g, lane, radius, radii, gauss_h);
    float4 nt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m.valid) nt = rec[m.p];
    const float n0 = nt.x, n1 = nt.y, n2 = nt.z, tt = nt.w;
    m.valid = m.valid && (n0 != 0.f || n1 != 0.f || n2 != 0.f);
    const float qx = m.qx, qy = m.qy, qz = m.qz, k = m.k;
    const float r2 = m.valid ? m.r2 : -1.f;
    // the frame: a = the axis where |n| is smallest (ties: the lowest), U = normalise(n x a), V = n x U
    const float a0 = fabsf(n0), a1 = fabsf(n1), a2 = fabsf(n2);
    float u0, u1, u2;
    if (a0 <= a1 && a0 <= a2) { u0 = 0.f; u1 = n2; u2 = -n1; }
    else if (a1 <= a2) { u0 = -n2; u1 = 0.f; u2 = n0; }
    else { u0 = n1; u1 = -n0; u2 = 0.f; }
    const float ulen = sqrtf(sq3(u0, u1, u2));
    if (m.valid) { u0 /= ulen; u1 /= ulen; u2 /= ulen; }
    const float v0 = n1 * u2 - n2 * u1, v1 = n2 * u0 - n0 * u2, v2 = n0 * u1 - n1 * u0;
    const float o0 = tt * n0, o1 = tt * n1, o2 = tt * n2;
    const float rinv = m.valid ? 1.f / m.r : 0.f;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    u32 cnt = 0;
    // m_ij = sum w u^i v^j; z_ij = sum w z u^i v^j
    float m00 = 0.f, m10 = 0.f, m01 = 0.f, m20 = 0.f, m11 = 0.f, m02 = 0.f, m30 = 0.f, m21 = 0.f, m12 = 0.f, m03 = 0.f;
    float m40 = 0.f, m31 = 0.f, m22 = 0.f, m13 = 0.f, m04 = 0.f;
    float z00 = 0.f, z10 = 0.f, z01 = 0.f, z20 = 0.f, z11 = 0.f, z02 = 0.f;
    walk_needed_leaves<false>(t, need, [&](const u32, const Leaf* record, const u64, const u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const float d2 = sq3(dx, dy, dz);
            if (d2 <= r2) {  // (a NaN padding point fails)
                const float w = expf(d2 * k);
                const float ex = dx - o0, ey = dy - o1, ez = dz - o2;
                const float u = ((ex * u0 + ey * u1) + ez * u2) * rinv;
                const float v = ((ex * v0 + ey * v1) + ez * v2) * rinv;
                const float z = ((ex * n0 + ey * n1) + ez * n2) * rinv;
                const float wu = w * u, wv = w * v, wz = w * z;
                const float uu = u * u, uv = u * v, vv = v * v;
                cnt += 1u;
                m00 += w; m10 += wu; m01 += wv;
                m20 += wu * u; m11 += wu * v; m02 += wv * v;
                m30 += wu * uu; m21 += wu * uv; m12 += wu * vv; m03 += wv * vv;
                m40 += (wu * u) * uu; m31 += (wu * u) * uv; m22 += (wu * u) * vv; m13 += (wu * v) * vv; m04 += (wv * v) * vv;
                z00 += wz; z10 += wz * u; z01 += wz * v;
                z20 += wz * uu; z11 += wz * uv; z02 += wz * vv;
            }
        }
    });
    if (!m.valid || cnt < 6u) return;
    // b b^T by monomial: rows (1, u, v, uu, uv, vv)
    const double a[21] = {m00, m10, m01, m20, m11, m02,   // 1 x (1, u, v, uu, uv, vv)
                          m20, m11, m30, m21, m12,        // u x (u, v, uu, uv, vv)
                          m02, m21, m12, m03,             // v x (v, uu, uv, vv)
                          m40, m31, m22,                  // uu x (uu, uv, vv)
                          m22, m13,                       // uv x (uv, vv)
                          m04};                           // vv x vv
    const double b[6] = {z00, z10, z01, z20, z11, z02};
    double c[6];
    if (!mls_cholesky(a, b, c)) return;
    const double r = m.r;
    const double lift = c[0] * r;
    const double e0 = static_cast<double>(o0) + lift * n0, e1 = static_cast<double>(o1) + lift * n1, e2 = static_cast<double>(o2) + lift * n2;
    const float d0 = static_cast<float>(e0), d1 = static_cast<float>(e1), d2 = static_cast<float>(e2);
    const u64 row = m.row, r3 = 3ull * row;
    if (out.points) {
        out.points[r3] = qx + d0;
        out.points[r3 + 1] = qy + d1;
        out.points[r3 + 2] = qz + d2;
    }
    if (out.disp) {
        out.disp[r3] = d0;
        out.disp[r3 + 1] = d1;
        out.disp[r3 + 2] = d2;
    }
    if (out.normals) {
        const double x = n0 - c[1] * u0 - c[2] * v0, y = n1 - c[1] * u1 - c[2] * v1, zz = n2 - c[1] * u2 - c[2] * v2;
        const double len = sqrt((x * x + y * y) + zz * zz);
        out.normals[r3] = static_cast<float>(x / len);
        out.normals[r3 + 1] = static_cast<float>(y / len);
        out.normals[r3 + 2] = static_cast<float>(zz / len);
    }
    if (out.curvatures) {
        const double hu = c[1], hv = c[2], huu = 2.0 * c[3] / r, huv = c[4] / r, hvv = 2.0 * c[5] / r;
        const double gg = 1.0 + hu * hu + hv * hv;
        const double big_k = (huu * hvv - huv * huv) / (gg * gg);
        const double big_h = ((1.0 + hv * hv) * huu - 2.0 * hu * hv * huv + (1.0 + hu * hu) * hvv) / (2.0 * gg * sqrt(gg));
        out.curvatures[2 * row] = static_cast<float>(big_h);
        out.curvatures[2 * row + 1] = static_cast<float>(big_k);
    }
    if (out.fit) out.fit[row] = 2u;
}

// the fit-0 values at the rows of the points that are not indexed (position_of = 0xFFFFFFFF: outside the voxel grid, NaN, +-inf), as
// k_range_moments_empty_rows; the point's own bits from the index's copy of the cloud
__global__ __launch_bounds__(256) void k_mls_unindexed_rows(const u32* __restrict__ pos_of, const float* __restrict__ xyz, u64 n_rows, MlsOut out)
{
    const u64 i = blockIdx.x * static_cast<u64>(blockDim.x) + threadIdx.x;
    if (i >= n_rows || pos_of[i] != 0xFFFFFFFFu) return;
    write_unchanged(out, i, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0u);
}

// A slice [sorted_first, sorted_first + sorted_count) of the curve order, clamped to the cloud (as pcpx_api.hip's): exactly the
// positions [lo, hi) are answered, and gc groups from group gf hold them
struct Slice {
    u64 lo, hi, gf, gc;
};
Slice slice_of(const Index& ix, u64 sorted_first, u64 sorted_count)
{
    const u64 n = ix.n;
    Slice s;
    s.lo = sorted_first < n ? sorted_first : n;
    s.hi = sorted_count > n - s.lo ? n : s.lo + sorted_count;
    s.gf = s.lo / GROUP;
    const u64 gend = (s.hi + GROUP - 1) / GROUP;
    s.gc = gend > s.gf ? gend - s.gf : 0;
    return s;
}

int check_mls_args(const char* what, float radius, float gauss_h, int order, const MlsOut& out)
{
    if (out.none()) {
        set_error("%s: every output is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!(gauss_h > 0.f)) {  // (false for NaN)
        set_error("%s: gauss_h must be > 0 (got %g)", what, static_cast<double>(gauss_h));
        return PCPX_ERR_INVALID;
    }
    if (order != 1 && order != 2) {
        set_error("%s: the order must be 1 or 2 (got %d)", what, order);
        return PCPX_ERR_INVALID;
    }
    return check_radius(what, radius);
}

// Both kernels over query groups [gf, gf + gc) of qv; d_rec: one float4 per position of those groups (order 2), indexed by position
int launch_mls(Index& ix, const QueryView& qv, bool self, u64 gf64, u64 gc, float radius, const float* d_radii, float gauss_h, int order,
               float4* d_rec, const MlsOut& out)
{
    if (gc == 0) return PCPX_OK;
    const u32 grid = grid_for_groups(gc);
    const u32 gf = static_cast<u32>(gf64), ge = static_cast<u32>(gf64 + gc);
    const dim3 block(64 * WAVES_PER_BLOCK);
    const TreeView t = ix.view();
    float4* rec = order == 2 ? d_rec : nullptr;
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (self) k_mls_plane<true><<<grid, block, 0, ix.stream>>>(t, qv, gf, ge, radius, d_radii, gauss_h, rec, out);
    else k_mls_plane<false><<<grid, block, 0, ix.stream>>>(t, qv, gf, ge, radius, d_radii, gauss_h, rec, out);
    if (order == 2) {
        if (self) k_mls_poly<true><<<grid, block, 0, ix.stream>>>(t, qv, gf, ge, radius, d_radii, gauss_h, rec, out);
        else k_mls_poly<false><<<grid, block, 0, ix.stream>>>(t, qv, gf, ge, radius, d_radii, gauss_h, rec, out);
    }
    return check_hip(hipGetLastError(), "k_mls launch", __FILE__, __LINE__);
}

// The projection for the curve positions of slice `sl`, by input row, on the handle's stream: what both self forms run.  The
// records of order 2 lie in the handle's scratch, one per curve position.
int mls_self(Index& ix, float radius, float gauss_h, int order, const Slice& sl, const MlsOut& d)
{
    int st;
    const bool unindexed = sl.lo == 0 && sl.hi == ix.n && ix.n != ix.n_in;  // the whole curve order: the rows of the points that are not indexed too
    const bool records = order == 2 && sl.gc != 0;
    Carve c;
    const size_t rec_off = records ? c.take((ix.n + GROUP) * sizeof(float4)) : 0;
    const size_t pos_of_off = unindexed ? c.take(ix.n_in * sizeof(u32)) : 0;
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    float4* rec = records ? reinterpret_cast<float4*>(base + rec_off) : nullptr;
    if (unindexed) {
        u32* position_of = reinterpret_cast<u32*>(base + pos_of_off);
        PCPX_HIP(hipMemsetAsync(position_of, 0xFF, ix.n_in * sizeof(u32), ix.stream));
        if ((st = launch_invert_perm(ix.d_perm, ix.n, position_of, ix.stream)) != PCPX_OK) return st;
        k_mls_unindexed_rows<<<blocks_of(ix.n_in, 256), 256, 0, ix.stream>>>(position_of, ix.d_xyz, ix.n_in, d);
        if ((st = check_hip(hipGetLastError(), "k_mls_unindexed_rows launch", __FILE__, __LINE__)) != PCPX_OK) return st;
    }
    QueryView qv = self_view(ix);
    qv.pos_lo = static_cast<u32>(sl.lo);
    qv.pos_hi = static_cast<u32>(sl.hi);
    return launch_mls(ix, qv, true, sl.gf, sl.gc, radius, nullptr, gauss_h, order, rec, d);
}

// Host outputs: one device block per asked output, `run` fills them, then the copies back and the wait
template <class Run>
int mls_staged(Staged& stage, u64 rows, const MlsOut& out, Run&& run)
{
    int st;
    MlsOut d;
    d.points = stage.alloc_for(out.points, rows * 3 * sizeof(float));
    d.disp = stage.alloc_for(out.disp, rows * 3 * sizeof(float));
    d.normals = stage.alloc_for(out.normals, rows * 3 * sizeof(float));
    d.curvatures = stage.alloc_for(out.curvatures, rows * 2 * sizeof(float));
    d.count = stage.alloc_for(out.count, rows * sizeof(u32));
    d.fit = stage.alloc_for(out.fit, rows * sizeof(u32));
    if ((st = stage.st) != PCPX_OK || (st = run(d)) != PCPX_OK) return st;
    stage.download_opt(out.points, d.points, rows * 3 * sizeof(float));
    stage.download_opt(out.disp, d.disp, rows * 3 * sizeof(float));
    stage.download_opt(out.normals, d.normals, rows * 3 * sizeof(float));
    stage.download_opt(out.curvatures, d.curvatures, rows * 2 * sizeof(float));
    stage.download_opt(out.count, d.count, rows * sizeof(u32));
    stage.download_opt(out.fit, d.fit, rows * sizeof(u32));
    return stage.wait();
}

MlsOut mls_out(float* points, float* disp, float* normals, float* curvatures, u32* count, u32* fit)
{
    MlsOut o;
    o.points = points;
    o.disp = disp;
    o.normals = normals;
    o.curvatures = curvatures;
    o.count = count;
    o.fit = fit;
    return o;
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_mls_project_self_dev(pcpx_index* h, float radius, float gauss_h, int order, uint64_t sorted_first, uint64_t sorted_count,
                              float* d_opt_points, float* d_opt_displacements, float* d_opt_normals, float* d_opt_curvatures,
                              uint32_t* d_opt_count, uint32_t* d_opt_fit)
{
    static const char* what = "pcpx_mls_project_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        const MlsOut d = mls_out(d_opt_points, d_opt_displacements, d_opt_normals, d_opt_curvatures, d_opt_count, d_opt_fit);
        if ((st = check_mls_args(what, radius, gauss_h, order, d)) != PCPX_OK) return st;
        return mls_self(*ix, radius, gauss_h, order, slice_of(*ix, sorted_first, sorted_count), d);
    });
}

int pcpx_mls_project_self(pcpx_index* h, float radius, float gauss_h, int order, float* opt_points, float* opt_displacements,
                          float* opt_normals, float* opt_curvatures, uint32_t* opt_count, uint32_t* opt_fit)
{
    static const char* what = "pcpx_mls_project_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        const MlsOut out = mls_out(opt_points, opt_displacements, opt_normals, opt_curvatures, opt_count, opt_fit);
        if ((st = check_mls_args(what, radius, gauss_h, order, out)) != PCPX_OK) return st;
        if (ix->n_in == 0) return PCPX_OK;
        return mls_staged(stage, ix->n_in, out, [&](const MlsOut& d) {
            return mls_self(*ix, radius, gauss_h, order, slice_of(*ix, 0, UINT64_MAX), d);
        });
    });
}

int pcpx_mls_project_batch(pcpx_index* h, const float* q_xyz, const float* radii, float radius, float gauss_h, int order, uint64_t nq,
                           float* opt_points, float* opt_displacements, float* opt_normals, float* opt_curvatures, uint32_t* opt_count,
                           uint32_t* opt_fit)
{
    static const char* what = "pcpx_mls_project_batch";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        const MlsOut out = mls_out(opt_points, opt_displacements, opt_normals, opt_curvatures, opt_count, opt_fit);
        if ((st = check_mls_args(what, radius, gauss_h, order, out)) != PCPX_OK) return st;
        if (nq > 0 && !q_xyz) {
            set_error("%s: q_xyz is NULL with nq = %llu", what, static_cast<unsigned long long>(nq));
            return PCPX_ERR_INVALID;
        }
        if (radii) {
            if (!(radius > 0.f)) {
                set_error("%s: with one radius per sphere `radius` is the one gauss_h belongs to and must be > 0 (got %g)", what,
                          static_cast<double>(radius));
                return PCPX_ERR_INVALID;
            }
            for (u64 i = 0; i < nq; ++i)
                if (!(radii[i] >= 0.f)) {
                    set_error("%s: radius %llu must be >= 0 (got %g)", what, static_cast<unsigned long long>(i), static_cast<double>(radii[i]));
                    return PCPX_ERR_INVALID;
                }
        }
        if (nq == 0) return PCPX_OK;
        const float* dq = stage.upload(q_xyz, nq * 3 * sizeof(float));
        const float* dr = stage.upload(radii, nq * sizeof(float));
        float4* rec = order == 2 ? stage.alloc<float4>((nq + GROUP) * sizeof(float4)) : nullptr;  // (the handle's scratch holds the sorted queries)
        QueryView qv;
        if ((st = stage.st) != PCPX_OK || (st = prepare_queries(*ix, dq, nq, qv)) != PCPX_OK) return st;
        return mls_staged(stage, nq, out, [&](const MlsOut& d) {
            return launch_mls(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, radius, dr, gauss_h, order, rec, d);
        });
    });
}

}  // extern "C"
