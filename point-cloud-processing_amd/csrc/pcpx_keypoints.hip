// pcpx_keypoints.hip -- keypoints of the indexed cloud (include/pcpx_keypoints.h): the local maxima of a
// per-point score over a radius, and the ISS detector as a thin layer on the features form of pcpx_range.hip.  A seventh form of
// the leaf-direct sphere walk of pcpx_device.h: its pair test is "within r AND the partner beats me", and it reads the partners'
// scores leaf by leaf the way it reads their coordinates.  Unlike pcpx_subsample.hip it needs no rounds: the answer for a point
// depends only on the scores in its own sphere, which nothing writes during the launch.  So it is one launch, a leaf's eight
// scores are one scalar load, and a beaten lane goes idle at once.
#include "pcpx_keep.h"
#include "pcpx_keypoints.h"

namespace pcpx {

namespace {

constexpr u32 KP_BLOCK = 256;

// The scores of a leaf's eight points by curve position: one 32-byte scalar load per leaf, beside its coordinate record.  NaN in
// a slot that holds no point and in a non-candidate's: a NaN beats nobody, and a non-candidate -- score below min_score, so below
// every candidate's -- could beat no candidate anyway, so the walk needs no min_score test.
struct Scores8 {
    float v[LEAF];
};
static_assert(sizeof(Scores8) == 4 * LEAF, "score record must be dense");

// One thread per leaf slot (npos = 8 nleaves of them) and per input row, whichever are more: the point's score from its input row
// into the leaf's score record, and keep = 0 for every input row (k_local_maxima writes the kept rows only, and the rows of
// points outside the grid are written here).
__global__ __launch_bounds__(KP_BLOCK) void k_maxima_prep(TreeView t, u32 npos, u32 rows, const float* __restrict__ score, float min_score,
                                                          Scores8* __restrict__ srec, uint8_t* __restrict__ keep)
{
    const u32 p = blockIdx.x * KP_BLOCK + threadIdx.x;
    if (p < rows) keep[p] = 0;
    if (p >= npos) return;
    float s = __builtin_nanf("");
    if (p < t.n) {
        const float mine = score[t.leaves[p / LEAF].id[p % LEAF]];
        if (mine >= min_score) s = mine;  // (false for a NaN score)
    }
    srec[p / LEAF].v[p % LEAF] = s;
}

// One wave per group of 64 curve-consecutive positions, one lane per candidate; the others idle (r2 = -1), and a group with no
// candidate returns after one load.  A partner's score and input index are scalars of the two leaf records.  A beaten lane sets
// r2 = -1: it passes no further distance test and asks for no further box.  A lane that is alive at the end has walked its whole
// sphere, so its count is complete.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_local_maxima(TreeView t, u32 group_end, float radius, u32 min_neighbours,
                                                                      const Scores8* __restrict__ srec, uint8_t* __restrict__ keep)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    float s = __builtin_nanf("");
    if (p < t.n) s = srec[p / LEAF].v[p % LEAF];
    const bool active = s == s;
    if (!any_lane(active)) return;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    if (active) c = lane_query<true>(t, QueryView{}, p);
    const float qx = c.x, qy = c.y, qz = c.z;
    const u32 row = c.row;
    float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    u32 cnt = 0;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
        const Scores8 sc = load_const(srec + leaf);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            if (sq3(dx, dy, dz) <= r2) {  // (a NaN padding point fails; so does every point once the lane is beaten)
                cnt += 1u;
                if (sc.v[j] > s || (sc.v[j] == s && lf.id[j] < row)) r2 = -1.f;  // (never the lane's own point; a NaN score fails both)
            }
        }
    });
    if (r2 >= 0.f && cnt >= min_neighbours) keep[row] = 1;
}

// saliency by input row from the features form's eigenvalues and counts (count 0: a point outside the grid, whose evals row is
// not read)
__global__ __launch_bounds__(KP_BLOCK) void k_iss_score(u32 rows, const float* __restrict__ evals, const u32* __restrict__ count, float gamma21,
                                                        float gamma32, float* __restrict__ saliency)
{
    const u32 i = blockIdx.x * KP_BLOCK + threadIdx.x;
    if (i >= rows) return;
    float s = __builtin_nanf("");
    const u32 n = count[i];
    if (n != 0u) {
        const float l0 = evals[3ull * i], l1 = evals[3ull * i + 1], l2 = evals[3ull * i + 2];
        if (l1 < gamma21 * l2 && l0 < gamma32 * l1) s = __fdiv_rn(l0, static_cast<float>(n));
    }
    saliency[i] = s;
}

// Where the local maxima's arrays lie in the handle's scratch, taken from the caller's Carve (the ISS call keeps its own arrays
// below them): the score records (one word per leaf slot; the scan's places, one word per input row, take their room once the walk
// is done) and the scan's tile sums.  The caller ensures the scratch for the whole Carve before anything is enqueued.
struct MaximaScratch {
    size_t words_at, sums_at;
    MaximaScratch(Carve& c, const Index& ix)
    {
        const u64 npos = static_cast<u64>(ix.nleaves) * LEAF, rows = ix.n_in;
        words_at = c.take((npos > rows ? npos : rows) * sizeof(u32));
        sums_at = c.take((scan_tiles(rows) + 1ull) * sizeof(u32));
    }
};

int check_maxima_args(const char* what, float radius, const char* radius_name, u32 flags, const void* keep)
{
    if (!(radius >= 0.f)) {  // (false for NaN)
        set_error("%s: the %s must be >= 0 (got %g)", what, radius_name, static_cast<double>(radius));
        return PCPX_ERR_INVALID;
    }
    if (flags != 0u) {
        set_error("%s: unknown flag bits 0x%x", what, flags);
        return PCPX_ERR_INVALID;
    }
    if (!keep) {
        set_error("%s: the keep array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}
int check_not_nan(const char* what, float v, const char* name)
{
    if (v == v) return PCPX_OK;
    set_error("%s: %s is NaN", what, name);
    return PCPX_ERR_INVALID;
}

// Everything is enqueued on the handle's stream.  Scratch of the handle: `at`, which the caller has ensured (no row: none needed).
int local_maxima_at(Index& ix, const MaximaScratch& at, const float* d_score, float radius, float min_score, u32 min_neighbours, uint8_t* d_keep,
                    u32* d_kept_rows, u64* d_kept_count)
{
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    if (rows == 0) {
        if (d_kept_count) PCPX_HIP(hipMemsetAsync(d_kept_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    char* base = static_cast<char*>(ix.d_scratch);
    Scores8* srec = reinterpret_cast<Scores8*>(base + at.words_at);
    u32* sums = reinterpret_cast<u32*>(base + at.sums_at);
    if (n > 0) {
        const TreeView t = ix.view();
        const u64 npos = static_cast<u64>(ix.nleaves) * LEAF;  // >= n
        const u64 groups = (n + GROUP - 1) / GROUP;
        k_maxima_prep<<<blocks_of(npos > rows ? npos : rows, KP_BLOCK), KP_BLOCK, 0, s>>>(t, static_cast<u32>(npos), static_cast<u32>(rows), d_score,
                                                                                         min_score, srec, d_keep);
        k_local_maxima<<<grid_for_groups(groups), 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, min_neighbours, srec, d_keep);
        PCPX_HIP(hipGetLastError());
    } else {
        PCPX_HIP(hipMemsetAsync(d_keep, 0, rows * sizeof(uint8_t), s));  // every point lies outside the voxel grid
    }
    // (the records are free by now: the scan's places)
    return count_and_compact_kept(d_keep, rows, reinterpret_cast<u32*>(srec), sums, d_kept_rows, d_kept_count, s);
}

int local_maxima_self(Index& ix, const float* d_score, float radius, float min_score, u32 min_neighbours, uint8_t* d_keep, u32* d_kept_rows,
                      u64* d_kept_count)
{
    Carve c;
    const MaximaScratch at(c, ix);
    if (const int st = ix.n_in ? ensure_scratch(ix, c.bytes()) : PCPX_OK) return st;
    return local_maxima_at(ix, at, d_score, radius, min_score, min_neighbours, d_keep, d_kept_rows, d_kept_count);
}

// The features form at the salient radius into the handle's scratch, the saliency, its local maxima at the other radius.  One Carve
// for its own arrays and the maxima's, ensured once: nothing moves under the arrays already written.
int iss_keypoints_self(Index& ix, float salient_radius, float non_max_radius, float gamma21, float gamma32, u32 min_neighbours, uint8_t* d_keep,
                       u32* d_kept_rows, u64* d_kept_count, float* d_saliency)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    if (rows == 0) return local_maxima_self(ix, nullptr, non_max_radius, 0.f, min_neighbours, d_keep, d_kept_rows, d_kept_count);
    Carve c;
    const size_t evals_at = c.take(rows * 3 * sizeof(float)), count_at = c.take(rows * sizeof(u32));
    const size_t saliency_at = d_saliency ? 0 : c.take(rows * sizeof(float));
    const MaximaScratch maxima(c, ix);
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    float* evals = reinterpret_cast<float*>(base + evals_at);
    u32* count = reinterpret_cast<u32*>(base + count_at);
    if (!d_saliency) d_saliency = reinterpret_cast<float*>(base + saliency_at);
    if (n != rows) PCPX_HIP(hipMemsetAsync(count, 0, rows * sizeof(u32), s));  // the rows of the points outside the voxel grid
    if (n > 0) {
        if ((st = launch_range_features(ix, self_view(ix), true, 0, (n + GROUP - 1) / GROUP, salient_radius, nullptr, evals, nullptr, nullptr, nullptr,
                                        count)) != PCPX_OK)
            return st;
    }
    k_iss_score<<<blocks_of(rows, KP_BLOCK), KP_BLOCK, 0, s>>>(static_cast<u32>(rows), evals, count, gamma21, gamma32, d_saliency);
    PCPX_HIP(hipGetLastError());
    return local_maxima_at(ix, maxima, d_saliency, non_max_radius, -std::numeric_limits<float>::infinity(), min_neighbours, d_keep, d_kept_rows,
                           d_kept_count);
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

int check_local_maxima(const char* what, const float* score, float radius, float min_score, u32 flags, const void* keep)
{
    int st;
    if ((st = check_maxima_args(what, radius, "radius", flags, keep)) != PCPX_OK) return st;
    if ((st = check_not_nan(what, min_score, "min_score")) != PCPX_OK) return st;
    if (!score) {
        set_error("%s: the score array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}
int check_iss(const char* what, float salient_radius, float non_max_radius, float gamma21, float gamma32, u32 flags, const void* keep)
{
    int st;
    if ((st = check_maxima_args(what, salient_radius, "salient radius", flags, keep)) != PCPX_OK) return st;
    if ((st = check_maxima_args(what, non_max_radius, "non-maximum radius", flags, keep)) != PCPX_OK) return st;
    if ((st = check_not_nan(what, gamma21, "gamma21")) != PCPX_OK) return st;
    return check_not_nan(what, gamma32, "gamma32");
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_local_maxima_self_dev(pcpx_index* h, const float* d_score, float radius, float min_score, uint32_t min_neighbours, uint32_t flags,
                               uint8_t* d_keep, uint32_t* d_opt_kept_rows, uint64_t* d_opt_kept_count)
{
    static const char* what = "pcpx_local_maxima_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_local_maxima(what, d_score, radius, min_score, flags, d_keep)) != PCPX_OK) return st;
        return booked_as_one_range_interval(*ix, [&] {
            return local_maxima_self(*ix, d_score, radius, min_score, min_neighbours, d_keep, d_opt_kept_rows, d_opt_kept_count);
        });
    });
}

int pcpx_local_maxima_self(pcpx_index* h, const float* score, float radius, float min_score, uint32_t min_neighbours, uint32_t flags,
                           uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count)
{
    static const char* what = "pcpx_local_maxima_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_local_maxima(what, score, radius, min_score, flags, keep)) != PCPX_OK) return st;
        if (opt_kept_count) *opt_kept_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        const float* dscore = stage.upload(score, rows * sizeof(float), true);  // (plain: measured, pcpx_stage.h)
        uint8_t* dk = stage.alloc<uint8_t>(rows * sizeof(uint8_t));
        u32* dr = stage.alloc_for(opt_kept_rows, rows * sizeof(u32));
        u64* dt = opt_kept_rows || opt_kept_count ? stage.alloc<u64>(sizeof(u64)) : nullptr;
        if ((st = stage.st) != PCPX_OK) return st;
        st = booked_as_one_range_interval(*ix, [&] { return local_maxima_self(*ix, dscore, radius, min_score, min_neighbours, dk, dr, dt); });
        if (st != PCPX_OK) return st;
        stage.download(keep, dk, rows * sizeof(uint8_t));
        return download_kept(stage, dt, dr, opt_kept_count, opt_kept_rows);
    });
}

int pcpx_iss_keypoints_self_dev(pcpx_index* h, float salient_radius, float non_max_radius, float gamma21, float gamma32, uint32_t min_neighbours,
                                uint32_t flags, uint8_t* d_keep, uint32_t* d_opt_kept_rows, uint64_t* d_opt_kept_count, float* d_opt_saliency)
{
    static const char* what = "pcpx_iss_keypoints_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_iss(what, salient_radius, non_max_radius, gamma21, gamma32, flags, d_keep)) != PCPX_OK) return st;
        return booked_as_one_range_interval(*ix, [&] {
            return iss_keypoints_self(*ix, salient_radius, non_max_radius, gamma21, gamma32, min_neighbours, d_keep, d_opt_kept_rows,
                                      d_opt_kept_count, d_opt_saliency);
        });
    });
}

int pcpx_iss_keypoints_self(pcpx_index* h, float salient_radius, float non_max_radius, float gamma21, float gamma32, uint32_t min_neighbours,
                            uint32_t flags, uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count, float* opt_saliency)
{
    static const char* what = "pcpx_iss_keypoints_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_iss(what, salient_radius, non_max_radius, gamma21, gamma32, flags, keep)) != PCPX_OK) return st;
        if (opt_kept_count) *opt_kept_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        uint8_t* dk = stage.alloc<uint8_t>(rows * sizeof(uint8_t));
        u32* dr = stage.alloc_for(opt_kept_rows, rows * sizeof(u32));
        u64* dt = opt_kept_rows || opt_kept_count ? stage.alloc<u64>(sizeof(u64)) : nullptr;
        float* ds = stage.alloc_for(opt_saliency, rows * sizeof(float));
        if ((st = stage.st) != PCPX_OK) return st;
        st = booked_as_one_range_interval(*ix, [&] {
            return iss_keypoints_self(*ix, salient_radius, non_max_radius, gamma21, gamma32, min_neighbours, dk, dr, dt, ds);
        });
        if (st != PCPX_OK) return st;
        stage.download(keep, dk, rows * sizeof(uint8_t));
        stage.download_opt(opt_saliency, ds, rows * sizeof(float));
        return download_kept(stage, dt, dr, opt_kept_count, opt_kept_rows);
    });
}

}  // extern "C"
