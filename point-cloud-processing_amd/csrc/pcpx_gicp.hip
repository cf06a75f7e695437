// pcpx_gicp.hip -- Generalized ICP on the indexed cloud (include/pcpx_gicp.h): the loop of pcpx_icp.hip
// (icp_loop_device: the exact partner search, the loop's rules, the Cholesky solve and the Cayley step) around the plane-to-plane
// sums of this file.
//   k_fixed_partial / k_fixed_final (pcpx_fixed_sum.h) over GicpSystem   per pair: S = C_t + R C_s R^T, its 3 x 3 Cholesky factor L,
//                     z = L^-1 r and K = L^-1 J by forward substitution, then K^T K, K^T z and z.z into the 29 float64 sums of the
//                     point-to-plane layout, in the fits' fixed order
// All float64, no FMA (-ffp-contract=off), every index a compile-time constant after unrolling.
#include "pcpx_device.h"
#include "pcpx_fixed_sum.h"
#include "pcpx_gicp.h"
#include "pcpx_plane_solve.h"
#include "pcpx_stage.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace pcpx {

namespace {

constexpr u32 GICP_TERMS = PLANE_A_TERMS + PLANE_B_TERMS + 2, GICP_STRIDE = 32;  // A, b, sum z.z, rows: the slots k_plane_solve reads

struct GicpIn {
    const float* s;           // the source
    const float* xyz;         // the target by input row
    const float* source_cov;  // by source row: 3 floats (a normal) or 6 (a covariance's upper triangle)
    const float* target_cov;  // by input row of the target, the same
    const uint2* pairs;       // {i, partner of i}, m of them
    u32 m, n_in;
    u32 covariances;          // PCPX_GICP_COVARIANCES or 0
    double keep;              // 1 - epsilon
    double o[3];
};

// where entry (r, c) of a symmetric 3 x 3 matrix sits among the 6 of its upper triangle: xx, xy, xz, yy, yz, zz
constexpr int sym_at(int r, int c) { return r <= c ? r * 3 - r * (r - 1) / 2 + (c - r) : c * 3 - c * (c - 1) / 2 + (r - c); }

// the matrix C of a row (its upper triangle), or false where the row has none
__device__ __forceinline__ bool gicp_matrix(const float* __restrict__ rows, u32 row, bool covariances, double keep, double (&c)[6])
{
    if (covariances) {
        bool fine = true;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const float v = rows[6ull * row + e];
            fine = fine && std::isfinite(v);
            c[e] = v;
        }
        return fine;
    }
    const double n[3] = {rows[3ull * row], rows[3ull * row + 1], rows[3ull * row + 2]};
    const double q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(q > 0.0 && q < std::numeric_limits<double>::infinity())) return false;  // (false for a NaN)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = r; k < 3; ++k) c[sym_at(r, k)] = (r == k ? 1.0 : 0.0) - (keep * (n[r] * n[k])) / q;
    }
    return true;
}

// v = L^-1 a, L lower triangular (l: 00, 10, 11, 20, 21, 22)
__device__ __forceinline__ void forward3(const double (&l)[6], double a0, double a1, double a2, double& v0, double& v1, double& v2)
{
    v0 = a0 / l[0];
    v1 = (a1 - l[1] * v0) / l[2];
    v2 = ((a2 - l[3] * v0) - l[4] * v1) / l[5];
}

// The sums of the plane-to-plane normal equations over the usable rows, in pcpx_fixed_sum.h's order; the totals go where
// k_plane_solve reads them.  Once the loop has stopped there are no rows: the launches still run, and leave zeros.
struct GicpSystem {
    static constexpr int TERMS = GICP_TERMS, STRIDE = GICP_STRIDE;
    GicpIn in;
    const double* pose;  // the round's pose
    const u32* done;
    double* sums;
    double T[12];  // (items() leaves the round's pose here for add())
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ u32 items()
    {
#pragma unroll
        for (int j = 0; j < 12; ++j) T[j] = pose[j];
        return *done ? 0u : in.m;
    }
    __device__ __forceinline__ void add(u32 i, double (&acc)[TERMS]) const
    {
        const u32 target = in.pairs[i].y;
        if (target >= in.n_in) return;  // (no partner)
        double cs[6], ct[6];
        if (!gicp_matrix(in.source_cov, i, in.covariances != 0u, in.keep, cs)) return;
        if (!gicp_matrix(in.target_cov, target, in.covariances != 0u, in.keep, ct)) return;
        // S = C_t + (R C_s) R^T, the upper triangle
        double mm[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) mm[r][c] = (T[4 * r] * cs[sym_at(0, c)] + T[4 * r + 1] * cs[sym_at(1, c)]) + T[4 * r + 2] * cs[sym_at(2, c)];
        }
        double sm[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = r; c < 3; ++c) sm[sym_at(r, c)] = ct[sym_at(r, c)] + ((mm[r][0] * T[4 * c] + mm[r][1] * T[4 * c + 1]) + mm[r][2] * T[4 * c + 2]);
        }
        // S = L L^T with the pivot rule of plane_cholesky
        constexpr double INF = std::numeric_limits<double>::infinity();
        double l[6];
        const double d0 = sm[0];
        bool ok = d0 > PLANE_PIVOT_FLOOR * sm[0] && d0 < INF;
        l[0] = std::sqrt(d0);
        l[1] = sm[1] / l[0];
        l[3] = sm[2] / l[0];
        const double d1 = sm[3] - l[1] * l[1];
        ok = ok && d1 > PLANE_PIVOT_FLOOR * sm[3] && d1 < INF;
        l[2] = std::sqrt(d1);
        l[4] = (sm[4] - l[3] * l[1]) / l[2];
        const double d2 = (sm[5] - l[3] * l[3]) - l[4] * l[4];
        ok = ok && d2 > PLANE_PIVOT_FLOOR * sm[5] && d2 < INF;
        l[5] = std::sqrt(d2);
        if (!ok) return;
        const double a = in.s[3ull * i], b = in.s[3ull * i + 1], c = in.s[3ull * i + 2];
        double y[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) y[r] = ((T[4 * r] * a + T[4 * r + 1] * b) + T[4 * r + 2] * c) + T[4 * r + 3];
        const double e0 = y[0] - static_cast<double>(in.xyz[3ull * target]), e1 = y[1] - static_cast<double>(in.xyz[3ull * target + 1]),
                     e2 = y[2] - static_cast<double>(in.xyz[3ull * target + 2]);
        const double u0 = y[0] - in.o[0], u1 = y[1] - in.o[1], u2 = y[2] - in.o[2];
        const double J[3][6] = {{0.0, u2, -u1, 1.0, 0.0, 0.0}, {-u2, 0.0, u0, 0.0, 1.0, 0.0}, {u1, -u0, 0.0, 0.0, 0.0, 1.0}};
        double z[3], K[3][6];
        forward3(l, e0, e1, e2, z[0], z[1], z[2]);
#pragma unroll
        for (int k = 0; k < 6; ++k) forward3(l, J[0][k], J[1][k], J[2][k], K[0][k], K[1][k], K[2][k]);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int k = r; k < 6; ++k) acc[plane_at(r, k)] += (K[0][r] * K[0][k] + K[1][r] * K[1][k]) + K[2][r] * K[2][k];
            acc[PLANE_A_TERMS + r] -= (K[0][r] * z[0] + K[1][r] * z[1]) + K[2][r] * z[2];
        }
        acc[PLANE_A_TERMS + PLANE_B_TERMS] += (z[0] * z[0] + z[1] * z[1]) + z[2] * z[2];
        acc[PLANE_A_TERMS + PLANE_B_TERMS + 1] += 1.0;
    }
    __device__ __forceinline__ void finish(u32 term, double sum) const { sums[term] = sum; }
};

// ---- the host side -------------------------------------------------------------------------------------------------------------------
int check_gicp(const char* what, const void* s, u64 m, float radius, u32 max_iterations, u32 flags, const void* source_cov, const void* target_cov,
               float epsilon, const void* transform)
{
    const int st = icp_check_arguments(what, s, m, radius, max_iterations, transform);
    if (st != PCPX_OK) return st;
    constexpr u32 known = PCPX_GICP_COVARIANCES | PCPX_GICP_ON_DEVICE;
    if (flags & ~known) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~known);
        return PCPX_ERR_INVALID;
    }
    if (!source_cov && m) {
        set_error("%s: the source covariance array is NULL with m = %llu", what, static_cast<unsigned long long>(m));
        return PCPX_ERR_INVALID;
    }
    if (!target_cov) {
        set_error("%s: the target covariance array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (flags & PCPX_GICP_COVARIANCES) {
        if (!(epsilon == 0.f)) {
            set_error("%s: epsilon must be 0 with PCPX_GICP_COVARIANCES (got %g)", what, static_cast<double>(epsilon));
            return PCPX_ERR_INVALID;
        }
    } else if (!(epsilon > 0.f && epsilon <= 1.f)) {  // (false for a NaN)
        set_error("%s: epsilon must be in (0, 1] (got %g)", what, static_cast<double>(epsilon));
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int enqueue_gicp_sums(void* ctx, const double* d_pose, const u32* d_done, double* d_sums, const u32* d_pairs, double* d_partial, hipStream_t s)
{
    GicpSystem sys{*static_cast<const GicpIn*>(ctx), d_pose, d_done, d_sums, {}};
    sys.in.pairs = reinterpret_cast<const uint2*>(d_pairs);
    fixed_sum(sys, d_partial, s);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

int gicp_device(Index& ix, const char* what, const float* d_s, u64 m, const double* d_pose, float radius, u32 max_iterations, u32 flags,
                const float* d_source_cov, const float* d_target_cov, float epsilon, const IcpLoopOut& out)
{
    GicpIn in{d_s, ix.d_xyz, d_source_cov, d_target_cov, nullptr, static_cast<u32>(m), static_cast<u32>(ix.n_in), flags & PCPX_GICP_COVARIANCES,
                   1.0 - static_cast<double>(epsilon),
                   {(static_cast<double>(ix.bbox[0]) + static_cast<double>(ix.bbox[3])) / 2.0,
                    (static_cast<double>(ix.bbox[1]) + static_cast<double>(ix.bbox[4])) / 2.0,
                    (static_cast<double>(ix.bbox[2]) + static_cast<double>(ix.bbox[5])) / 2.0}};
    const IcpSumsStep step{enqueue_gicp_sums, &in, 3u};
    return icp_loop_device(ix, what, d_s, m, d_pose, radius, max_iterations, step, out);
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_gicp_rigid(pcpx_index* h, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t max_iterations, uint32_t flags,
                    const float* source_cov, const float* target_cov, float epsilon, double* out_transform, uint32_t* opt_out_status,
                    uint32_t* opt_out_iterations, uint32_t* opt_out_last_count, uint32_t* opt_out_count_trace, double* opt_out_rms_trace,
                    uint32_t* opt_out_partner)
{
    static const char* what = "pcpx_gicp_rigid";
    const int st = check_gicp(what, s, m, radius, max_iterations, flags, source_cov, target_cov, epsilon, out_transform);
    if (st != PCPX_OK) return st;
    if (flags & PCPX_GICP_ON_DEVICE) {  // every array is the caller's device array: enqueued, no wait, nothing read back
        return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
            const IcpLoopOut out{out_transform, opt_out_status, opt_out_iterations, opt_out_last_count, opt_out_count_trace, opt_out_rms_trace,
                                 opt_out_partner};
            return gicp_device(*ix, what, s, m, opt_pose, radius, max_iterations, flags, source_cov, target_cov, epsilon, out);
        });
    }
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        // the small outputs as one block: the transform, the rms trace, then the words and the count trace
        struct Small {
            double transform[16], rms[PCPX_ICP_MAX_ITERATIONS];
            u32 status, iterations, last_count, pad, count[PCPX_ICP_MAX_ITERATIONS];
        };
        const size_t width = (flags & PCPX_GICP_COVARIANCES) ? 6 : 3;
        std::vector<Small> host(1);
        const float* ds = stage.upload(m ? s : nullptr, m * 3 * sizeof(float));
        const double* dpose = stage.upload(opt_pose, 16 * sizeof(double));
        const float* dcs = stage.upload(m ? source_cov : nullptr, m * width * sizeof(float));
        const float* dct = stage.upload(ix->n_in ? target_cov : nullptr, ix->n_in * width * sizeof(float));  // (an empty target: nothing is read)
        u32* dpart = m ? stage.alloc_for(opt_out_partner, m * sizeof(u32)) : nullptr;
        Small* d = stage.alloc<Small>(sizeof(Small));
        if (stage.st != PCPX_OK) return stage.st;
        const IcpLoopOut out{d->transform, &d->status, &d->iterations, &d->last_count, d->count, d->rms, dpart};
        const int r = gicp_device(*ix, what, ds, m, dpose, radius, max_iterations, flags, dcs, dct, epsilon, out);
        if (r != PCPX_OK) return r;
        stage.download(host.data(), d, sizeof(Small));
        if (dpart) stage.download(opt_out_partner, dpart, m * sizeof(u32));
        if (stage.wait() != PCPX_OK) return stage.st;
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
