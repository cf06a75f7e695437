// pcpx_outliers.hip -- outlier removal of the indexed cloud (include/pcpx_outliers.h): the cloud's
// resolution, the statistical filter, the radius filter and the density filter, each enqueued from its first kernel to its last.
// Mostly composition: the mean distances are k_knn's (its fused epilogue, or the multi-pass path for k > 32), the counts are
// k_range's, the two float64 sums are pcpx_fixed_sum.h's, the kept rows are pcpx_keep.h's.  What is new is the tail between them
// (the two sum types, the kernel that forms mean, std and the cut, the keep kernels) and that the density filter's radius stays
// a word of device memory: k_range_radius_at (pcpx_range.hip) reads it there.
#include "pcpx_fixed_sum.h"
#include "pcpx_keep.h"
#include "pcpx_outliers.h"

#include <cmath>
#include <limits>

namespace pcpx {

namespace {

constexpr u32 OUT_BLOCK = 256;

// What the tail leaves in the handle's scratch: the totals of the two sums, the stats of a caller who passed none, the cut (the
// statistical filter's threshold or the density filter's radius) as the float32 word the next kernel reads.
struct TailState {
    double s1, m, s2;
    double stats[4];
    float cut;
};

// usable: indexed -- the row of a point outside the voxel grid holds the NaN it was filled with -- and a finite mean distance
__device__ __forceinline__ bool usable(float d) { return __builtin_isfinite(d); }

// S1 = sum (double)d_i and m = the number of usable rows (an exact integer in a double), the input rows being the items
struct DistSum {
    static constexpr int TERMS = 2;
    static constexpr u32 STRIDE = 2;
    const float* dist;
    u32 rows;
    TailState* state;
    __device__ bool live() const { return true; }
    __device__ u32 items() const { return rows; }
    __device__ void add(u32 j, double* acc) const
    {
        const float d = dist[j];
        if (usable(d)) {
            acc[0] += static_cast<double>(d);
            acc[1] += 1.0;
        }
    }
    __device__ void finish(u32 t, double total) const { (t == 0 ? state->s1 : state->m) = total; }
};

// S2 = sum e e, e = (double)d_i - mean, with the mean = S1 / m of the totals that DistSum's finish() left in device memory: every
// thread forms the same quotient once, in items().  One rounding each for e, the product and the add (-ffp-contract=off).
struct DeviationSum {
    static constexpr int TERMS = 1;
    static constexpr u32 STRIDE = 1;
    const float* dist;
    u32 rows;
    TailState* state;
    double mean;
    __device__ bool live() const { return true; }
    __device__ u32 items()
    {
        mean = state->s1 / state->m;
        return rows;
    }
    __device__ void add(u32 j, double* acc) const
    {
        const float d = dist[j];
        if (usable(d)) {
            const double e = static_cast<double>(d) - mean;
            acc[0] += e * e;
        }
    }
    __device__ void finish(u32, double total) const { state->s2 = total; }
};

enum Mode : int { RESOLUTION = 0, STATISTICAL = 1, RADIUS = 2, DENSITY = 3 };

// One thread: mean, std, the cut and the stats words from the three totals.  m = 0: 0 / 0, so mean, std and the cut are NaN.
__global__ void k_outlier_stats(TailState* __restrict__ state, int mode, float param, double* __restrict__ stats)
{
    const double m = state->m;
    const double mean = state->s1 / m;
    double std = __builtin_nan("");
    if (m >= 2.0) std = sqrt(state->s2 / (m - 1.0));
    else if (m == 1.0) std = 0.0;
    float cut = __builtin_nanf("");
    if (mode == STATISTICAL) {
        const double scaled = static_cast<double>(param) * std;
        cut = static_cast<float>(mean + scaled);
    } else if (mode == DENSITY) {
        cut = static_cast<float>(static_cast<double>(param) * mean);
    }
    state->cut = cut;
    stats[0] = mean;
    stats[1] = std;
    stats[2] = static_cast<double>(cut);
    stats[3] = m;
}

// keep_i = usable_i && d_i <= cut, in float32 (false for a NaN cut)
__global__ __launch_bounds__(OUT_BLOCK) void k_outlier_keep_near(const float* __restrict__ dist, u32 rows, const TailState* __restrict__ state,
                                                                uint8_t* __restrict__ keep)
{
    const u32 i = blockIdx.x * OUT_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const float d = dist[i];
    keep[i] = usable(d) && d <= state->cut ? 1 : 0;
}

// keep_i = count_i >= at_least (at_least >= 1: the count of a row outside the voxel grid is the 0 it was filled with)
__global__ __launch_bounds__(OUT_BLOCK) void k_outlier_keep_dense(const u32* __restrict__ count, u32 rows, u32 at_least, uint8_t* __restrict__ keep)
{
    const u32 i = blockIdx.x * OUT_BLOCK + threadIdx.x;
    if (i < rows) keep[i] = count[i] >= at_least ? 1 : 0;
}

struct Request {
    Mode mode;
    u32 k = 0;
    float eps = 0.f;
    float param = 0.f;   // std_ratio (STATISTICAL), radius_scale (DENSITY)
    float radius = 0.f;  // RADIUS
    u32 min_neighbours = 0;
    bool resolves() const { return mode != RADIUS; }
    bool counts() const { return mode == RADIUS || mode == DENSITY; }
    bool keeps() const { return mode != RESOLUTION; }
};
// device arrays; any but keep (of a call that keeps) and stats (of the resolution) may be null
struct Outputs {
    uint8_t* keep = nullptr;
    u32* kept_rows = nullptr;
    u64* kept_count = nullptr;
    float* mean_dist = nullptr;
    u32* count = nullptr;
    double* stats = nullptr;
};

// Everything is enqueued on the handle's stream; the scratch is the handle's, ensured once before the first launch.
int outliers_self(Index& ix, const Request& rq, Outputs o)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    const u64 groups = (n + GROUP - 1) / GROUP;
    const bool multipass = rq.resolves() && rq.k > 32;
    // A caller who wants no counts gets the at-least form of the sphere walk, which writes the keep decision itself and stops a lane
    // at the bound; the counts of one who wants them are the count form's, and the keep decision is taken from them.
    const bool at_least_form = rq.counts() && !o.count;
    const u32 at_least = rq.min_neighbours > 1u ? rq.min_neighbours : 1u;
    Carve c;
    const size_t state_at = c.take(sizeof(TailState));
    size_t partial_at = 0, dist_at = 0, idx_at = 0, found_at = 0, place_at = 0, sums_at = 0;
    if (rq.resolves()) {
        partial_at = c.take(FIT_BLOCKS * DistSum::STRIDE * sizeof(double));
        if (!o.mean_dist) dist_at = c.take(rows * sizeof(float));
        if (multipass) {  // the rows and their counts: n_in (k + 1) 4 bytes
            idx_at = c.take(rows * rq.k * sizeof(u32));
            found_at = c.take(rows * sizeof(u32));
        }
    }
    if (rq.keeps()) {
        place_at = c.take(rows * sizeof(u32));
        sums_at = c.take((scan_tiles(rows) + 1ull) * sizeof(u32));
    }
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    TailState* state = reinterpret_cast<TailState*>(base + state_at);
    if (!o.mean_dist) o.mean_dist = reinterpret_cast<float*>(base + dist_at);
    if (!o.stats) o.stats = state->stats;
    const u32 rows32 = static_cast<u32>(rows);

    if (rq.resolves()) {
        // the rows of the points outside the voxel grid: NaN, which no kernel below takes for usable
        if (n != rows && (st = launch_fill_f32(o.mean_dist, rows, std::numeric_limits<float>::quiet_NaN(), s)) != PCPX_OK) return st;
        KnnOutputs ko;
        ko.meandist = o.mean_dist;
        ko.pos_lo = 0;
        ko.pos_hi = static_cast<u32>(n);
        if (multipass) {
            ko.idx = reinterpret_cast<u32*>(base + idx_at);
            ko.cnt = reinterpret_cast<u32*>(base + found_at);
        }
        if ((st = launch_knn(ix, self_view(ix), true, 0, groups, rq.k, rq.eps, ko)) != PCPX_OK) return st;
        double* partial = reinterpret_cast<double*>(base + partial_at);
        fixed_sum(DistSum{o.mean_dist, rows32, state}, partial, s);
        fixed_sum(DeviationSum{o.mean_dist, rows32, state, 0.0}, partial, s);
        k_outlier_stats<<<1, 1, 0, s>>>(state, rq.mode, rq.param, o.stats);
        PCPX_HIP(hipGetLastError());
    }
    if (rq.counts()) {
        // (points outside the grid are in no sphere and have none of their own: count 0, not kept)
        if (n != rows) PCPX_HIP(at_least_form ? hipMemsetAsync(o.keep, 0, rows * sizeof(uint8_t), s) : hipMemsetAsync(o.count, 0, rows * sizeof(u32), s));
        QueryView qv = self_view(ix);
        qv.pos_lo = 0;
        qv.pos_hi = static_cast<u32>(n);
        const float* radius_at = rq.mode == DENSITY ? &state->cut : nullptr;
        if (at_least_form) st = launch_range_at_least_self(ix, qv, 0, groups, rq.radius, radius_at, at_least, o.keep);
        else if (radius_at) st = launch_range_count_self_radius_at(ix, qv, 0, groups, radius_at, o.count);
        else st = launch_range_count(ix, qv, true, 0, groups, rq.radius, nullptr, o.count);
        if (st != PCPX_OK) return st;
    }
    if (!rq.keeps()) return PCPX_OK;
    if (rows == 0) {
        if (o.kept_count) PCPX_HIP(hipMemsetAsync(o.kept_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    if (!rq.counts()) k_outlier_keep_near<<<blocks_of(rows, OUT_BLOCK), OUT_BLOCK, 0, s>>>(o.mean_dist, rows32, state, o.keep);
    else if (!at_least_form) k_outlier_keep_dense<<<blocks_of(rows, OUT_BLOCK), OUT_BLOCK, 0, s>>>(o.count, rows32, at_least, o.keep);
    PCPX_HIP(hipGetLastError());
    return count_and_compact_kept(o.keep, rows, reinterpret_cast<u32*>(base + place_at), reinterpret_cast<u32*>(base + sums_at), o.kept_rows,
                                  o.kept_count, s);
}

// One interval for the whole call (what it launches through other modules books nothing of its own): the PCPX_K_RANGE family for
// the radius filter, the PCPX_K_KNN family for the others, whose time is the neighbour search's.
int booked_as_one_interval(Index& ix, const Request& rq, const Outputs& o)
{
    ProfileScope prof(ix, rq.mode == RADIUS ? PCPX_K_RANGE : PCPX_K_KNN);
    const bool profiling = ix.profiling;
    ix.profiling = false;
    const int st = outliers_self(ix, rq, o);
    ix.profiling = profiling;
    return st;
}

int check_request(const char* what, const Request& rq, u32 flags, const void* required, const char* required_name)
{
    if (flags & ~PCPX_OUTLIERS_ON_DEVICE) {
        set_error("%s: unknown flag bits 0x%x", what, flags);
        return PCPX_ERR_INVALID;
    }
    if (!required) {
        set_error("%s: the %s array is NULL", what, required_name);
        return PCPX_ERR_INVALID;
    }
    if (rq.resolves() && rq.k == 0) {
        set_error("%s: k must be at least 1", what);
        return PCPX_ERR_INVALID;
    }
    if (rq.mode == STATISTICAL && !std::isfinite(rq.param)) {
        set_error("%s: std_ratio must be finite (got %g)", what, static_cast<double>(rq.param));
        return PCPX_ERR_INVALID;
    }
    if (rq.mode == DENSITY && !(rq.param >= 0.f && std::isfinite(rq.param))) {
        set_error("%s: radius_scale must be finite and >= 0 (got %g)", what, static_cast<double>(rq.param));
        return PCPX_ERR_INVALID;
    }
    if (rq.mode == RADIUS && !(rq.radius >= 0.f)) {  // (false for NaN)
        set_error("%s: the radius must be >= 0 (got %g)", what, static_cast<double>(rq.radius));
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

// Both forms of an entry point.  PCPX_OUTLIERS_ON_DEVICE: the caller's arrays are the device path's.  Otherwise a block of the
// handle's pool for every array the caller asked for, the same device path, the copies back and the wait.
int run(pcpx_index* h, const char* what, const Request& rq, u32 flags, const Outputs& o, const void* required, const char* required_name)
{
    if (flags & PCPX_OUTLIERS_ON_DEVICE) {
        return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
            if (const int st = check_request(what, rq, flags, required, required_name)) return st;
            return booked_as_one_interval(*ix, rq, o);
        });
    }
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_request(what, rq, flags, required, required_name)) != PCPX_OK) return st;
        if (o.kept_count) *o.kept_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) {  // (no usable row)
            const double nan = std::numeric_limits<double>::quiet_NaN();
            if (o.stats) o.stats[0] = o.stats[1] = o.stats[2] = nan, o.stats[3] = 0.0;
            return PCPX_OK;
        }
        Outputs d;
        d.keep = stage.alloc_for(o.keep, rows * sizeof(uint8_t));
        d.kept_rows = stage.alloc_for(o.kept_rows, rows * sizeof(u32));
        d.kept_count = o.kept_rows || o.kept_count ? stage.alloc<u64>(sizeof(u64)) : nullptr;
        d.mean_dist = stage.alloc_for(o.mean_dist, rows * sizeof(float));
        d.count = stage.alloc_for(o.count, rows * sizeof(u32));
        d.stats = stage.alloc_for(o.stats, 4 * sizeof(double));
        if ((st = stage.st) != PCPX_OK) return st;
        if ((st = booked_as_one_interval(*ix, rq, d)) != PCPX_OK) return st;
        stage.download_opt(o.keep, d.keep, rows * sizeof(uint8_t));
        stage.download_opt(o.mean_dist, d.mean_dist, rows * sizeof(float));
        stage.download_opt(o.count, d.count, rows * sizeof(u32));
        stage.download_opt(o.stats, d.stats, 4 * sizeof(double));
        return download_kept(stage, d.kept_count, d.kept_rows, o.kept_count, o.kept_rows);
    });
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_outliers_resolution_self(pcpx_index* h, uint32_t k, float eps, uint32_t flags, float* opt_mean_dist, double* stats)
{
    Request rq{RESOLUTION};
    rq.k = k;
    rq.eps = eps;
    Outputs o;
    o.mean_dist = opt_mean_dist;
    o.stats = stats;
    return run(h, "pcpx_outliers_resolution_self", rq, flags, o, stats, "stats");
}

int pcpx_outliers_statistical_self(pcpx_index* h, uint32_t k, float eps, float std_ratio, uint32_t flags, uint8_t* keep,
                                   uint32_t* opt_kept_rows, uint64_t* opt_kept_count, float* opt_mean_dist, double* opt_stats)
{
    Request rq{STATISTICAL};
    rq.k = k;
    rq.eps = eps;
    rq.param = std_ratio;
    Outputs o;
    o.keep = keep;
    o.kept_rows = opt_kept_rows;
    o.kept_count = opt_kept_count;
    o.mean_dist = opt_mean_dist;
    o.stats = opt_stats;
    return run(h, "pcpx_outliers_statistical_self", rq, flags, o, keep, "keep");
}

int pcpx_outliers_radius_self(pcpx_index* h, float radius, uint32_t min_neighbours, uint32_t flags, uint8_t* keep, uint32_t* opt_kept_rows,
                              uint64_t* opt_kept_count, uint32_t* opt_count)
{
    Request rq{RADIUS};
    rq.radius = radius;
    rq.min_neighbours = min_neighbours;
    Outputs o;
    o.keep = keep;
    o.kept_rows = opt_kept_rows;
    o.kept_count = opt_kept_count;
    o.count = opt_count;
    return run(h, "pcpx_outliers_radius_self", rq, flags, o, keep, "keep");
}

int pcpx_outliers_density_self(pcpx_index* h, uint32_t k, float eps, float radius_scale, uint32_t min_neighbours, uint32_t flags, uint8_t* keep,
                               uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint32_t* opt_count, double* opt_stats)
{
    Request rq{DENSITY};
    rq.k = k;
    rq.eps = eps;
    rq.param = radius_scale;
    rq.min_neighbours = min_neighbours;
    Outputs o;
    o.keep = keep;
    o.kept_rows = opt_kept_rows;
    o.kept_count = opt_kept_count;
    o.count = opt_count;
    o.stats = opt_stats;
    return run(h, "pcpx_outliers_density_self", rq, flags, o, keep, "keep");
}

}  // extern "C"
