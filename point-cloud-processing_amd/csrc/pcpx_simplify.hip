// pcpx_simplify.hip -- hierarchy simplification (Pauly et al.; include/pcp/algorithm/hierarchy_simplification.hpp:63-149 of
// the reference) on the GPU, level by level.
//
// The reference pops clusters from a FIFO queue: split a cluster by the plane through its mean normal to its largest
// eigenvector while it holds more than cluster_size points or its variation exceeds var_max, else keep the point nearest
// to its mean.  Queue order is breadth-first, left child before right, so one level of the tree is one step here:
//
//   the points are one permutation, float4 {x, y, z, input index bits}, ping-ponged between two buffers; every active
//   cluster owns a range [b, e) of it for its whole life (the partition is stable and nothing is compacted), and the
//   active clusters of a level are listed in ascending b -- which is the reference's queue order within the level;
//   the work of a level is cut into chunks of HS_CHUNK points of one cluster (a cluster of L points has ceil(L/CHUNK)
//   chunks; the chunks of all clusters are numbered through an exclusive scan), one wavefront per chunk:
//     k_hs_sum       per-chunk double sums of x, y, z
//     k_hs_mean      one wave per cluster: the chunk partials in chunk order -> the mean
//     k_hs_moments   per-chunk centred scatter sums (6 accumulators, double)
//     k_hs_decide    one wave per cluster: the sums in chunk order, a double Jacobi eigen solve, var, the split wish,
//                    the plane (n with its largest-magnitude component positive, d = mu . n)
//     k_hs_count     per chunk: points with f = p . n - d <= 0, and the (d2, index) minimum to the mean
//     k_hs_resolve   one wave per cluster: left counts scanned over the chunks, the representative; a wished split that
//                    leaves one side empty makes the cluster a leaf
//     scan           {children, leaves} per cluster -> next-level slots and output slots
//     k_hs_emit      one thread per cluster: leaf -> its representative's input index at the next output slot; split ->
//                    the two children (left first) and their chunk counts
//     k_hs_scatter   per chunk of a split cluster: the stable partition into the other buffer (ballot prefixes)
//     scan, k_hs_tail  chunk offsets of the next level; output total, active clusters, chunks
// The host reads three counters per level.  Every reduction runs in a fixed order (lane-strided sums, then a butterfly),
// and nothing uses atomics, so two runs give the same bits.  The leaves of a level come out in ascending b and the levels
// in order, so the output is the reference's queue order without a sort.
#include "pcpx_internal.h"
#include "pcpx_scan.h"

#include <algorithm>
#include <cmath>

namespace pcpx {

namespace {

constexpr int HS_WAVE = 64;
constexpr int HS_ITEMS = 8;
constexpr u32 HS_CHUNK = HS_WAVE * HS_ITEMS;  // points per chunk
constexpr int HS_BLOCK = 256;
constexpr int HS_WPB = HS_BLOCK / HS_WAVE;

// per active cluster of the level being processed
struct ClusterState {
    double mx, my, mz;   // mean
    double nx, ny, nz;   // splitting normal (largest eigenvector, sign-normalised)
    double d;            // mu . n
    u32 wants;           // N > cluster_size || var > var_max
    u32 split;           // wants and both sides non-empty
    u32 nl;              // points with f <= 0
    u32 rep;             // input index of the point nearest to the mean
};

struct Ctl {
    u64 out;       // leaves emitted so far
    u64 clusters;  // active clusters of the next level
    u64 chunks;    // their chunks
    u32 bad;       // a non-finite input coordinate
    u32 pad;
};

__device__ __forceinline__ u32 lane_id() { return threadIdx.x & (HS_WAVE - 1); }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = HS_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, HS_WAVE);
    return v;
}

__device__ __forceinline__ u32 wave_sum_u32(u32 v)
{
#pragma unroll
    for (int o = HS_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, HS_WAVE);
    return v;
}

// (d2, index) minimum, smaller index on equal d2
__device__ __forceinline__ void better(double& d2, u32& idx, double od2, u32 oidx)
{
    if (od2 < d2 || (od2 == d2 && oidx < idx)) d2 = od2, idx = oidx;
}

__device__ __forceinline__ void wave_min(double& d2, u32& idx)
{
#pragma unroll
    for (int o = HS_WAVE / 2; o > 0; o >>= 1) {
        const double od2 = __shfl_xor(d2, o, HS_WAVE);
        const u32 oidx = __shfl_xor(idx, o, HS_WAVE);
        better(d2, idx, od2, oidx);
    }
}

// the cluster of chunk j: ch0 holds K + 1 strictly increasing offsets (every cluster has a chunk)
__device__ __forceinline__ u32 cluster_of(const u64* __restrict__ ch0, u32 K, u64 j)
{
    u32 lo = 0, hi = K;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (ch0[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct ChunkRange {
    u32 k;      // cluster
    u32 b, e;   // cluster range
    u32 p0, p1; // this chunk's points
    u32 c;      // chunk number within the cluster
};

__device__ __forceinline__ ChunkRange chunk_range(const uint2* __restrict__ cl, const u64* __restrict__ ch0, u32 K, u64 j)
{
    ChunkRange r;
    r.k = cluster_of(ch0, K, j);
    const uint2 be = cl[r.k];
    r.b = be.x, r.e = be.y;
    r.c = static_cast<u32>(j - ch0[r.k]);
    r.p0 = r.b + r.c * HS_CHUNK;
    r.p1 = r.e - r.p0 < HS_CHUNK ? r.e : r.p0 + HS_CHUNK;
    return r;
}

__device__ __forceinline__ u64 wave_global() { return static_cast<u64>(blockIdx.x) * HS_WPB + (threadIdx.x >> 6); }
__device__ __forceinline__ u64 wave_stride() { return static_cast<u64>(gridDim.x) * HS_WPB; }

__device__ __forceinline__ double plane_f(const float4 p, const ClusterState& s)
{
    return static_cast<double>(p.x) * s.nx + static_cast<double>(p.y) * s.ny + static_cast<double>(p.z) * s.nz - s.d;
}

__device__ __forceinline__ double d2_to_mean(const float4 p, const ClusterState& s)
{
    const double dx = static_cast<double>(p.x) - s.mx, dy = static_cast<double>(p.y) - s.my, dz = static_cast<double>(p.z) - s.mz;
    return dx * dx + dy * dy + dz * dz;
}

// ---- setup ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(HS_BLOCK) void k_hs_pack(const float* __restrict__ xyz, u32 n, float4* __restrict__ rec, Ctl* __restrict__ ctl)
{
    const u32 i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3ull * i], y = xyz[3ull * i + 1], z = xyz[3ull * i + 2];
    if (!isfinite(x) || !isfinite(y) || !isfinite(z)) ctl->bad = 1u;  // (every writer stores the same word)
    rec[i] = make_float4(x, y, z, __uint_as_float(i));
}

__global__ void k_hs_init(u32 n, uint2* __restrict__ cl, u64* __restrict__ ch0, Ctl* __restrict__ ctl)
{
    cl[0] = make_uint2(0u, n);
    ch0[0] = 0;
    ch0[1] = (static_cast<u64>(n) + HS_CHUNK - 1) / HS_CHUNK;
    ctl->out = 0;
    ctl->clusters = 1;
    ctl->chunks = ch0[1];
    ctl->bad = 0;
    ctl->pad = 0;
}

// ---- one level --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(HS_BLOCK) void k_hs_sum(const float4* __restrict__ rec, const uint2* __restrict__ cl, const u64* __restrict__ ch0,
                                                     u32 K, u64 C, double* __restrict__ part)
{
    for (u64 j = wave_global(); j < C; j += wave_stride()) {
        const ChunkRange r = chunk_range(cl, ch0, K, j);
        double sx = 0, sy = 0, sz = 0;
#pragma unroll
        for (int i = 0; i < HS_ITEMS; ++i) {
            const u32 p = r.p0 + i * HS_WAVE + lane_id();
            if (p < r.p1) {
                const float4 q = rec[p];
                sx += q.x, sy += q.y, sz += q.z;
            }
        }
        sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
        if (lane_id() == 0) {
            double* o = part + 6 * j;
            o[0] = sx, o[1] = sy, o[2] = sz;
        }
    }
}

__global__ __launch_bounds__(HS_BLOCK) void k_hs_mean(const uint2* __restrict__ cl, const u64* __restrict__ ch0, u32 K, const double* __restrict__ part,
                                                      ClusterState* __restrict__ st)
{
    for (u64 k = wave_global(); k < K; k += wave_stride()) {
        const u64 c0 = ch0[k], c1 = ch0[k + 1];
        double sx = 0, sy = 0, sz = 0;
        for (u64 c = c0 + lane_id(); c < c1; c += HS_WAVE) {
            const double* q = part + 6 * c;
            sx += q[0], sy += q[1], sz += q[2];
        }
        sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
        if (lane_id() == 0) {
            const uint2 be = cl[k];
            const double N = static_cast<double>(be.y - be.x);
            st[k].mx = sx / N, st[k].my = sy / N, st[k].mz = sz / N;
        }
    }
}

__global__ __launch_bounds__(HS_BLOCK) void k_hs_moments(const float4* __restrict__ rec, const uint2* __restrict__ cl, const u64* __restrict__ ch0,
                                                         u32 K, u64 C, const ClusterState* __restrict__ st, double* __restrict__ part)
{
    for (u64 j = wave_global(); j < C; j += wave_stride()) {
        const ChunkRange r = chunk_range(cl, ch0, K, j);
        const double mx = st[r.k].mx, my = st[r.k].my, mz = st[r.k].mz;
        double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
#pragma unroll
        for (int i = 0; i < HS_ITEMS; ++i) {
            const u32 p = r.p0 + i * HS_WAVE + lane_id();
            if (p < r.p1) {
                const float4 q = rec[p];
                const double dx = static_cast<double>(q.x) - mx, dy = static_cast<double>(q.y) - my, dz = static_cast<double>(q.z) - mz;
                xx += dx * dx, xy += dx * dy, xz += dx * dz;
                yy += dy * dy, yz += dy * dz, zz += dz * dz;
            }
        }
        xx = wave_sum(xx), xy = wave_sum(xy), xz = wave_sum(xz);
        yy = wave_sum(yy), yz = wave_sum(yz), zz = wave_sum(zz);
        if (lane_id() == 0) {
            double* o = part + 6 * j;
            o[0] = xx, o[1] = xy, o[2] = xz, o[3] = yy, o[4] = yz, o[5] = zz;
        }
    }
}

// One Jacobi rotation of the symmetric 3x3 a (entries named) zeroing a_pq; v accumulates the rotations (columns are
// eigenvectors).  Written per pair so that every index is a compile-time constant (no private arrays, no scratch).
#define HS_JACOBI_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                      \
    do {                                                                                            \
        if (apq != 0.0) {                                                                           \
            const double theta = (aqq - app) / (2.0 * apq);                                         \
            const double at = fabs(theta);                                                          \
            double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));                    \
            if (theta < 0.0) t = -t;                                                                \
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                    \
            app -= t * apq;                                                                         \
            aqq += t * apq;                                                                         \
            apq = 0.0;                                                                              \
            const double rp = arp, rq = arq;                                                        \
            arp = c * rp - s * rq;                                                                  \
            arq = s * rp + c * rq;                                                                  \
            double vp, vq;                                                                          \
            vp = v0p, vq = v0q, v0p = c * vp - s * vq, v0q = s * vp + c * vq;                       \
            vp = v1p, vq = v1q, v1p = c * vp - s * vq, v1q = s * vp + c * vq;                       \
            vp = v2p, vq = v2q, v2p = c * vp - s * vq, v2q = s * vp + c * vq;                       \
        }                                                                                           \
    } while (0)

// eigen decomposition of the symmetric matrix [[xx xy xz] [xy yy yz] [xz yz zz]]: eigenvalues w0 <= w1 <= w2 and the
// eigenvector of w2 (unit length)
__device__ void eig3_double(double xx, double xy, double xz, double yy, double yz, double zz, double& w0, double& w1, double& w2, double& ex,
                            double& ey, double& ez)
{
    double a00 = xx, a11 = yy, a22 = zz, a01 = xy, a02 = xz, a12 = yz;
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
    for (int sweep = 0; sweep < 24; ++sweep) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        const double diag = fabs(a00) + fabs(a11) + fabs(a22);
        if (off == 0.0 || off <= 1e-22 * diag) break;
        HS_JACOBI_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (p, q, r) = (0, 1, 2): a_r p = a02, a_r q = a12
        HS_JACOBI_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2, 1): a_r p = a01, a_r q = a21
        HS_JACOBI_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2, 0): a_r p = a10, a_r q = a20
    }
    // sort (value, column) ascending; the columns travel as three scalars each
    double l0 = a00, l1 = a11, l2 = a22;
    double c0x = v00, c0y = v10, c0z = v20, c1x = v01, c1y = v11, c1z = v21, c2x = v02, c2y = v12, c2z = v22;
#define HS_SWAP_COL(la, lb, ax, ay, az, bx, by, bz)                                              \
    if (lb < la) {                                                                              \
        double tmp = la; la = lb; lb = tmp;                                                     \
        tmp = ax, ax = bx, bx = tmp;                                                            \
        tmp = ay, ay = by, by = tmp;                                                            \
        tmp = az, az = bz, bz = tmp;                                                            \
    }
    HS_SWAP_COL(l0, l1, c0x, c0y, c0z, c1x, c1y, c1z)
    HS_SWAP_COL(l1, l2, c1x, c1y, c1z, c2x, c2y, c2z)
    HS_SWAP_COL(l0, l1, c0x, c0y, c0z, c1x, c1y, c1z)
#undef HS_SWAP_COL
    w0 = l0, w1 = l1, w2 = l2;
    const double len = sqrt(c2x * c2x + c2y * c2y + c2z * c2z);
    ex = c2x / len, ey = c2y / len, ez = c2z / len;
}

__global__ __launch_bounds__(HS_BLOCK) void k_hs_decide(const uint2* __restrict__ cl, const u64* __restrict__ ch0, u32 K, const double* __restrict__ part,
                                                        u64 cluster_size, double var_max, ClusterState* __restrict__ st)
{
    for (u64 k = wave_global(); k < K; k += wave_stride()) {
        const u64 c0 = ch0[k], c1 = ch0[k + 1];
        double m[6] = {0, 0, 0, 0, 0, 0};
        for (u64 c = c0 + lane_id(); c < c1; c += HS_WAVE) {
            const double* q = part + 6 * c;
#pragma unroll
            for (int t = 0; t < 6; ++t) m[t] += q[t];
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) m[t] = wave_sum(m[t]);
        if (lane_id() != 0) continue;
        double w0, w1, w2, nx, ny, nz;
        eig3_double(m[0], m[1], m[2], m[3], m[4], m[5], w0, w1, w2, nx, ny, nz);
        const double var = w0 / (w0 + w1 + w2);  // NaN for an all-zero scatter: never a split by itself
        const uint2 be = cl[k];
        const u64 N = be.y - be.x;
        ClusterState& s = st[k];
        s.wants = (N > cluster_size || var > var_max) ? 1u : 0u;
        // sign: the component of largest magnitude positive (the first on a tie)
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        if (big < 0.0) nx = -nx, ny = -ny, nz = -nz;
        s.nx = nx, s.ny = ny, s.nz = nz;
        s.d = s.mx * nx + s.my * ny + s.mz * nz;
    }
}

__global__ __launch_bounds__(HS_BLOCK) void k_hs_count(const float4* __restrict__ rec, const uint2* __restrict__ cl, const u64* __restrict__ ch0,
                                                       u32 K, u64 C, const ClusterState* __restrict__ st, u32* __restrict__ cnt,
                                                       double* __restrict__ best_d2, u32* __restrict__ best_idx)
{
    for (u64 j = wave_global(); j < C; j += wave_stride()) {
        const ChunkRange r = chunk_range(cl, ch0, K, j);
        const ClusterState s = st[r.k];
        u32 left = 0;
        double bd = __builtin_inf();
        u32 bi = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < HS_ITEMS; ++i) {
            const u32 p = r.p0 + i * HS_WAVE + lane_id();
            if (p < r.p1) {
                const float4 q = rec[p];
                if (s.wants) left += plane_f(q, s) <= 0.0 ? 1u : 0u;
                better(bd, bi, d2_to_mean(q, s), __float_as_uint(q.w));
            }
        }
        left = wave_sum_u32(left);
        wave_min(bd, bi);
        if (lane_id() == 0) {
            cnt[j] = left;
            best_d2[j] = bd;
            best_idx[j] = bi;
        }
    }
}

// cnt[chunk] -> left points before the chunk within its cluster (in place); the cluster's verdict; pk[k] = {children, leaves}
__global__ __launch_bounds__(HS_BLOCK) void k_hs_resolve(const uint2* __restrict__ cl, const u64* __restrict__ ch0, u32 K, u32* __restrict__ cnt,
                                                         const double* __restrict__ best_d2, const u32* __restrict__ best_idx,
                                                         ClusterState* __restrict__ st, u64* __restrict__ pk)
{
    for (u64 k = wave_global(); k < K; k += wave_stride()) {
        const u32 lane = lane_id();
        const u64 c0 = ch0[k], c1 = ch0[k + 1];
        u32 carry = 0;
        double bd = __builtin_inf();
        u32 bi = 0xFFFFFFFFu;
        for (u64 base = c0; base < c1; base += HS_WAVE) {
            const u64 c = base + lane;
            const u32 v = c < c1 ? cnt[c] : 0u;
            if (c < c1) better(bd, bi, best_d2[c], best_idx[c]);
            u32 incl = v;
#pragma unroll
            for (int o = 1; o < HS_WAVE; o <<= 1) {
                const u32 up = __shfl_up(incl, o, HS_WAVE);
                if (static_cast<int>(lane) >= o) incl += up;
            }
            if (c < c1) cnt[c] = carry + incl - v;
            carry += __shfl(incl, HS_WAVE - 1, HS_WAVE);
        }
        wave_min(bd, bi);
        if (lane != 0) continue;
        const uint2 be = cl[k];
        const u32 N = be.y - be.x;
        ClusterState& s = st[k];
        const u32 split = (s.wants && carry > 0 && carry < N) ? 1u : 0u;
        s.split = split;
        s.nl = carry;
        s.rep = bi;
        pk[k] = split ? 2ull : (1ull << 32);
    }
}

// after the exclusive scan of pk: leaves to the output, children to the next level
__global__ __launch_bounds__(HS_BLOCK) void k_hs_emit(const uint2* __restrict__ cl, u32 K, const ClusterState* __restrict__ st,
                                                      const u64* __restrict__ pk, const Ctl* __restrict__ ctl, u32* __restrict__ out_idx,
                                                      uint2* __restrict__ cl_next, u64* __restrict__ nch_next)
{
    const u32 k = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (k >= K) return;
    const u64 slot = pk[k];
    const ClusterState& s = st[k];
    if (!s.split) {
        out_idx[ctl->out + (slot >> 32)] = s.rep;
        return;
    }
    const uint2 be = cl[k];
    const u32 c = static_cast<u32>(slot & 0xFFFFFFFFull);
    const u32 mid = be.x + s.nl;
    cl_next[c] = make_uint2(be.x, mid);
    cl_next[c + 1] = make_uint2(mid, be.y);
    nch_next[c] = (static_cast<u64>(s.nl) + HS_CHUNK - 1) / HS_CHUNK;
    nch_next[c + 1] = (static_cast<u64>(be.y - mid) + HS_CHUNK - 1) / HS_CHUNK;
}

// stable partition of the split clusters' chunks: left points to [b, b + nl), right ones to [b + nl, e), input order kept
__global__ __launch_bounds__(HS_BLOCK) void k_hs_scatter(const float4* __restrict__ rec, const uint2* __restrict__ cl, const u64* __restrict__ ch0,
                                                         u32 K, u64 C, const ClusterState* __restrict__ st, const u32* __restrict__ lofs,
                                                         float4* __restrict__ rec_out)
{
    for (u64 j = wave_global(); j < C; j += wave_stride()) {
        const ChunkRange r = chunk_range(cl, ch0, K, j);
        const ClusterState s = st[r.k];
        if (!s.split) continue;
        const u32 lane = lane_id();
        const u64 below = (1ull << lane) - 1ull;
        const u32 left_before = lofs[j];
        u32 lpos = r.b + left_before;
        u32 rpos = r.b + s.nl + (r.c * HS_CHUNK - left_before);
#pragma unroll
        for (int i = 0; i < HS_ITEMS; ++i) {
            const u32 p = r.p0 + i * HS_WAVE + lane;
            const bool valid = p < r.p1;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            bool left = false;
            if (valid) {
                q = rec[p];
                left = plane_f(q, s) <= 0.0;
            }
            const u64 ml = __ballot(valid && left);
            const u64 mr = __ballot(valid && !left);
            if (valid) {
                const u32 dst = left ? lpos + __popcll(ml & below) : rpos + __popcll(mr & below);
                rec_out[dst] = q;
            }
            lpos += __popcll(ml);
            rpos += __popcll(mr);
        }
    }
}

__global__ void k_hs_tail(u32 K, const u64* __restrict__ pk, const u64* __restrict__ ch0_next, Ctl* __restrict__ ctl)
{
    const u64 t = pk[K];
    const u64 kn = t & 0xFFFFFFFFull;
    ctl->out += t >> 32;
    ctl->clusters = kn;
    ctl->chunks = ch0_next[kn];
}

__global__ __launch_bounds__(HS_BLOCK) void k_hs_gather(const float* __restrict__ xyz, const u32* __restrict__ idx, u32 m, float* __restrict__ out_xyz,
                                                        u32* __restrict__ out_idx)
{
    const u32 i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 s = idx[i];
    out_xyz[3ull * i] = xyz[3 * s];
    out_xyz[3ull * i + 1] = xyz[3 * s + 1];
    out_xyz[3ull * i + 2] = xyz[3 * s + 2];
    if (out_idx) out_idx[i] = idx[i];
}

// the wave kernels stride over their chunks / clusters: 64 K blocks of four waves fill the card many times over
u32 wave_blocks(u64 waves)
{
    const u64 b = (waves + HS_WPB - 1) / HS_WPB;
    return static_cast<u32>(b < 65536 ? (b > 0 ? b : 1) : 65536);
}
u32 thread_blocks(u64 threads) { return static_cast<u32>((threads + HS_BLOCK - 1) / HS_BLOCK); }

}  // namespace

int hierarchy_device(const float* d_xyz, u64 n, u64 cluster_size, double var_max, hipStream_t s, DevPool& pool, float* d_out_xyz, u32* d_out_idx,
                     u64 capacity, u64* out_count, HierarchyTimes* times)
{
    *out_count = 0;
    if (cluster_size == 0 || !(var_max >= 0.0)) {
        set_error("pcpx_hierarchy_simplification: cluster_size must be > 0 and var_max >= 0 (not NaN)");
        return PCPX_ERR_INVALID;
    }
    if (n >= 0xFFFFFFFFull) {
        set_error("pcpx_hierarchy_simplification: more than 2^32 - 2 points");
        return PCPX_ERR_INVALID;
    }
    if (n == 0) return PCPX_OK;
    if (!d_xyz) {
        set_error("pcpx_hierarchy_simplification: null points");
        return PCPX_ERR_INVALID;
    }
    const double vmax = static_cast<double>(static_cast<float>(var_max));  // the reference compares with (float)var_max
    const u32 n32 = static_cast<u32>(n);
    const u64 max_chunks = n + (n + HS_CHUNK - 1) / HS_CHUNK;  // sum over clusters of ceil(L / CHUNK) <= n / CHUNK + clusters
    const u64 tiles = scan_tiles(n + 1);
    DevBuf rec0(pool), rec1(pool), cl0(pool), cl1(pool), ch00(pool), ch01(pool), stb(pool), pkb(pool), sums(pool), part(pool), cnt(pool),
        bd2(pool), bidx(pool), outi(pool), ctlb(pool);
    int st;
    if ((st = rec0.alloc(n * sizeof(float4))) != PCPX_OK || (st = rec1.alloc(n * sizeof(float4))) != PCPX_OK ||
        (st = cl0.alloc(n * sizeof(uint2))) != PCPX_OK || (st = cl1.alloc(n * sizeof(uint2))) != PCPX_OK ||
        (st = ch00.alloc((n + 1) * sizeof(u64))) != PCPX_OK || (st = ch01.alloc((n + 1) * sizeof(u64))) != PCPX_OK ||
        (st = stb.alloc(n * sizeof(ClusterState))) != PCPX_OK || (st = pkb.alloc((n + 1) * sizeof(u64))) != PCPX_OK ||
        (st = sums.alloc(std::max<u64>(tiles, 64) * sizeof(u64))) != PCPX_OK || (st = part.alloc(max_chunks * 6 * sizeof(double))) != PCPX_OK ||
        (st = cnt.alloc(max_chunks * sizeof(u32))) != PCPX_OK || (st = bd2.alloc(max_chunks * sizeof(double))) != PCPX_OK ||
        (st = bidx.alloc(max_chunks * sizeof(u32))) != PCPX_OK || (st = outi.alloc(n * sizeof(u32))) != PCPX_OK ||
        (st = ctlb.alloc(sizeof(Ctl))) != PCPX_OK) {
        set_error("pcpx_hierarchy_simplification: out of device memory for %llu points", static_cast<unsigned long long>(n));
        return st;
    }
    float4* rec[2] = {rec0.as<float4>(), rec1.as<float4>()};
    uint2* cl[2] = {cl0.as<uint2>(), cl1.as<uint2>()};
    u64* ch0[2] = {ch00.as<u64>(), ch01.as<u64>()};
    ClusterState* cs = stb.as<ClusterState>();
    u64* pk = pkb.as<u64>();
    Ctl* ctl = ctlb.as<Ctl>();
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (times) {
        for (auto& e : ev) PCPX_HIP(hipEventCreate(&e));
    }
    struct EventsGone {
        hipEvent_t* e;
        ~EventsGone()
        {
            for (int q = 0; q < 3; ++q)
                if (e[q]) (void)hipEventDestroy(e[q]);
        }
    } events_gone{ev};
    if (times) PCPX_HIP(hipEventRecord(ev[0], s));
    k_hs_init<<<1, 1, 0, s>>>(n32, cl[0], ch0[0], ctl);
    k_hs_pack<<<thread_blocks(n), HS_BLOCK, 0, s>>>(d_xyz, n32, rec[0], ctl);
    PCPX_HIP(hipGetLastError());
    Ctl h{};
    PCPX_HIP(hipMemcpyAsync(&h, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    PCPX_HIP(hipStreamSynchronize(s));
    if (h.bad) {
        set_error("pcpx_hierarchy_simplification: a point has a non-finite coordinate");
        return PCPX_ERR_INVALID;
    }
    u64 K = 1, C = h.chunks;
    int cur = 0, levels = 0;
    while (K > 0) {
        const int nxt = cur ^ 1;
        const u32 K32 = static_cast<u32>(K);
        k_hs_sum<<<wave_blocks(C), HS_BLOCK, 0, s>>>(rec[cur], cl[cur], ch0[cur], K32, C, part.as<double>());
        k_hs_mean<<<wave_blocks(K), HS_BLOCK, 0, s>>>(cl[cur], ch0[cur], K32, part.as<double>(), cs);
        k_hs_moments<<<wave_blocks(C), HS_BLOCK, 0, s>>>(rec[cur], cl[cur], ch0[cur], K32, C, cs, part.as<double>());
        k_hs_decide<<<wave_blocks(K), HS_BLOCK, 0, s>>>(cl[cur], ch0[cur], K32, part.as<double>(), cluster_size, vmax, cs);
        k_hs_count<<<wave_blocks(C), HS_BLOCK, 0, s>>>(rec[cur], cl[cur], ch0[cur], K32, C, cs, cnt.as<u32>(), bd2.as<double>(), bidx.as<u32>());
        k_hs_resolve<<<wave_blocks(K), HS_BLOCK, 0, s>>>(cl[cur], ch0[cur], K32, cnt.as<u32>(), bd2.as<double>(), bidx.as<u32>(), cs, pk);
        PCPX_HIP(hipGetLastError());
        PCPX_HIP(hipMemsetAsync(pk + K, 0, sizeof(u64), s));
        if ((st = exclusive_scan_in_place<u64>(pk, K + 1, sums.as<u64>(), s)) != PCPX_OK) return st;
        // the next level has at most min(2K, n) clusters; their chunk counts, zero beyond, scanned with one entry more
        const u64 m = std::min<u64>(2 * K, n) + 1;
        PCPX_HIP(hipMemsetAsync(ch0[nxt], 0, m * sizeof(u64), s));
        k_hs_emit<<<thread_blocks(K), HS_BLOCK, 0, s>>>(cl[cur], K32, cs, pk, ctl, outi.as<u32>(), cl[nxt], ch0[nxt]);
        k_hs_scatter<<<wave_blocks(C), HS_BLOCK, 0, s>>>(rec[cur], cl[cur], ch0[cur], K32, C, cs, cnt.as<u32>(), rec[nxt]);
        PCPX_HIP(hipGetLastError());
        if ((st = exclusive_scan_in_place<u64>(ch0[nxt], m, sums.as<u64>(), s)) != PCPX_OK) return st;
        k_hs_tail<<<1, 1, 0, s>>>(K32, pk, ch0[nxt], ctl);
        PCPX_HIP(hipGetLastError());
        PCPX_HIP(hipMemcpyAsync(&h, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
        K = h.clusters, C = h.chunks;
        cur = nxt;
        ++levels;
    }
    const u64 m = h.out;
    *out_count = m;
    if (times) PCPX_HIP(hipEventRecord(ev[1], s));
    const bool fits = d_out_xyz && m <= capacity;
    if (fits) {
        k_hs_gather<<<thread_blocks(m), HS_BLOCK, 0, s>>>(d_xyz, outi.as<u32>(), static_cast<u32>(m), d_out_xyz, d_out_idx);
        PCPX_HIP(hipGetLastError());
    }
    if (times) {
        PCPX_HIP(hipEventRecord(ev[2], s));
        PCPX_HIP(hipEventSynchronize(ev[2]));
        PCPX_HIP(hipEventElapsedTime(&times->levels_ms, ev[0], ev[1]));
        PCPX_HIP(hipEventElapsedTime(&times->gather_ms, ev[1], ev[2]));
        times->levels = levels;
    }
    // the scratch goes back to the pool on return: nothing that reads it may still be queued
    PCPX_HIP(hipStreamSynchronize(s));
    if (!fits) {
        set_error("pcpx_hierarchy_simplification: %llu points are kept", static_cast<unsigned long long>(m));
        return PCPX_ERR_CAPACITY;
    }
    return PCPX_OK;
}

}  // namespace pcpx

using namespace pcpx;

static int hierarchy_params_of(const pcpx_hierarchy_params* params, u64& cluster_size, double& var_max)
{
    if (!params || params->struct_size != sizeof(pcpx_hierarchy_params)) {
        set_error("pcpx_hierarchy_simplification: params missing or params->struct_size mismatch");
        return PCPX_ERR_INVALID;
    }
    cluster_size = params->cluster_size;
    var_max = params->var_max;
    if (cluster_size == 0 || !(var_max >= 0.0)) {
        set_error("pcpx_hierarchy_simplification: cluster_size must be > 0 and var_max >= 0 (not NaN)");
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

extern "C" {

int pcpx_hierarchy_simplification_dev(const float* d_xyz, uint64_t n, const pcpx_hierarchy_params* params, int device, void* stream,
                                      float* d_out_xyz, uint32_t* d_opt_out_idx, uint64_t capacity, uint64_t* out_count)
{
    if (!out_count) return PCPX_ERR_INVALID;
    *out_count = 0;
    u64 cluster_size = 0;
    double var_max = 0;
    int st = hierarchy_params_of(params, cluster_size, var_max);
    if (st != PCPX_OK) return st;
    return on_shared(device, "pcpx_hierarchy_simplification_dev", [&](DeviceShared& sh) -> int {
        return hierarchy_device(d_xyz, n, cluster_size, var_max, static_cast<hipStream_t>(stream), sh.pool, d_out_xyz, d_opt_out_idx, capacity,
                                out_count);
    });
}

int pcpx_hierarchy_simplification(const float* xyz, uint64_t n, const pcpx_hierarchy_params* params, int device, float* out_xyz,
                                  uint32_t* opt_out_idx, uint64_t capacity, uint64_t* out_count)
{
    if (!out_count) return PCPX_ERR_INVALID;
    *out_count = 0;
    u64 cluster_size = 0;
    double var_max = 0;
    int st = hierarchy_params_of(params, cluster_size, var_max);
    if (st != PCPX_OK) return st;
    if (n == 0) return PCPX_OK;
    if (!xyz || n >= 0xFFFFFFFFull) {
        set_error("pcpx_hierarchy_simplification: null points or more than 2^32 - 2 of them");
        return PCPX_ERR_INVALID;
    }
    return on_shared(device, "pcpx_hierarchy_simplification", [&](DeviceShared& sh) -> int {
        PooledStream ps;
        PCPX_HIP(pooled_stream_get(&ps.s));
        const hipStream_t s = ps.s;
        const u64 cap = out_xyz ? std::min<u64>(capacity, n) : 0;
        DevBuf dp(sh.pool), dv(sh.pool), di(sh.pool);
        int r;
        if ((r = dp.alloc(n * 3 * sizeof(float))) != PCPX_OK || (cap > 0 && (r = dv.alloc(cap * 3 * sizeof(float))) != PCPX_OK) ||
            (cap > 0 && opt_out_idx && (r = di.alloc(cap * sizeof(u32))) != PCPX_OK))
            return r;
        if ((r = upload_pageable(dp.p, xyz, n * 3 * sizeof(float), s)) != PCPX_OK) return r;
        r = hierarchy_device(dp.as<float>(), n, cluster_size, var_max, s, sh.pool, cap > 0 ? dv.as<float>() : nullptr, di.as<u32>(), cap, out_count);
        if (r != PCPX_OK) return r;
        if (*out_count) {
            PCPX_HIP(hipMemcpyAsync(out_xyz, dv.p, *out_count * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
            if (opt_out_idx) PCPX_HIP(hipMemcpyAsync(opt_out_idx, di.p, *out_count * sizeof(u32), hipMemcpyDeviceToHost, s));
        }
        PCPX_HIP(hipStreamSynchronize(s));
        return PCPX_OK;
    });
}

}  // extern "C"
