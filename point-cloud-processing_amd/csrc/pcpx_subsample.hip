// pcpx_subsample.hip -- Poisson-disk subsampling of the indexed cloud (include/pcpx_subsample.h): the kept set
// of the greedy loop in ascending key(i) = fmix32(i ^ seed), found by rounds of the leaf-direct sphere walk of pcpx_device.h (one
// lane per UNDECIDED point, lane-per-range leaves) over one state word per CURVE POSITION; a second walk gives every dropped point
// its owner, and the passes after it turn states into the keep mask by input row and the ascending list of kept rows.
//
// The state words: UNDECIDED -> KEPT or DROPPED, once; a position that holds no indexed point is DROPPED from the start.  In a
// round an undecided point i looks at every partner j ~ i of smaller key: one that is KEPT drops i; else one that is UNDECIDED
// blocks i; else (every such partner is DROPPED) i is kept.
//
// Coherence: the words are written by other workgroups, on other XCDs, within the round launch, so every access to them there is
// an agent-scope atomic (relaxed: no other data is handed over through them), and the stores are vector stores.  The update is in
// place and needs no order, because the transitions are monotone and a decision only rests on FINAL words:
//   - KEPT or DROPPED, once read, is what the word holds for ever; a stale read can only show UNDECIDED where the word is final
//     by now, and that can only block a lane that could have decided: it delays, it never changes a decision.
//   - i is stored KEPT only after it read DROPPED for every smaller-key partner, and DROPPED only after it read KEPT for one; by
//     induction over ascending key these are the greedy loop's decisions, whatever the schedule.  So the fixed point is K.
//   - Progress: the undecided point of smallest key has only final partners of smaller key, and a launch sees every store of the
//     launches before it: every round decides at least that point.  Against the synchronous form (every lane reads the words as they
//     were when the round began: tests/subsample_model.py) a round here reads words that are at least as far, so by induction over
//     the rounds it has decided at least what the synchronous form has: never more rounds than that.
#include "pcpx_keep.h"
#include "pcpx_subsample.h"

namespace pcpx {

namespace {

constexpr u32 UNDECIDED = 0u, KEPT = 1u, DROPPED = 2u;
constexpr u32 SS_BLOCK = 256;
constexpr u32 ROUND_BATCH = PCPX_SUBSAMPLE_ROUND_BATCH;  // rounds between two reads of the counter (measured: DESIGN.md section 18)

__device__ __forceinline__ u32 state_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void state_store(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct States8 {
    u32 v[LEAF];
};

// one thread per leaf slot (npos = 8 nleaves of them)
__global__ __launch_bounds__(SS_BLOCK) void k_subsample_init(u32 n, u32 npos, u32* __restrict__ state)
{
    const u32 p = blockIdx.x * SS_BLOCK + threadIdx.x;
    if (p < npos) state[p] = p < n ? UNDECIDED : DROPPED;
}

// One round: one wave per group of 64 curve-consecutive positions, one lane per undecided point; the others idle (r2 = -1), and a
// group with no undecided lane returns at once.  A partner's key is arithmetic on the leaf record's scalar index; of a leaf where
// some lane has a smaller-key partner inside its sphere the eight state words are ONE vector load (lane l reads slot l & 7) and two
// ballots.  A lane that is dropped goes idle at once; a blocked lane walks on, since a KEPT partner may still drop it in this round.
// decided: += the lanes this launch decided, one atomic per wave.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_subsample_round(TreeView t, u32 group_end, float radius, u32 seed, u32* state, u32* decided)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool active = p < t.n && state_load(state + p) == UNDECIDED;
    if (!any_lane(active)) return;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    if (active) c = lane_query<true>(t, QueryView{}, p);
    const float qx = c.x, qy = c.y, qz = c.z;
    const u32 key = fmix32(c.row ^ seed);
    float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    bool blocked = false;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
        u32 earlier = 0;  // bit j: slot j is inside this lane's sphere and has a smaller key (never the lane's own point: keys are distinct)
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            if (sq3(dx, dy, dz) <= r2 && fmix32(lf.id[j] ^ seed) < key) earlier |= 1u << j;  // (a NaN padding point fails)
        }
        if (any_lane(earlier != 0u)) {
            const u32 s = state_load(state + leaf * LEAF + (lane & (LEAF - 1u)));  // (every lane is active here: the walk's control flow is wave-uniform)
            const u32 kept = static_cast<u32>(__builtin_amdgcn_ballot_w64(s == KEPT)) & 0xFFu;
            const u32 undecided = static_cast<u32>(__builtin_amdgcn_ballot_w64(s == UNDECIDED)) & 0xFFu;
            if (earlier & kept) r2 = -1.f;  // dropped: nothing more is needed
            else if (earlier & undecided) blocked = true;
        }
    });
    const bool dropped = active && r2 < 0.f;
    const bool done = active && (dropped || !blocked);
    if (done) state_store(state + p, dropped ? DROPPED : KEPT);
    const u64 who = __builtin_amdgcn_ballot_w64(done);
    if (lane == 0 && who != 0ull) __hip_atomic_fetch_add(decided, static_cast<u32>(__builtin_popcountll(who)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The owners, in a launch after the rounds: the same walk with every indexed lane that is not KEPT active.  Nothing writes the
// state words in this launch, so a leaf's eight are one scalar load beside its record.  A lane keeps the minimum of
// (d2 bits << 32 | input index) over the KEPT points in its sphere (the bits of a float >= 0 order as the float does) and needs
// no box beyond the best d2 so far (<=: a tie on d2 may still win by index).  A group of kept lanes only ends at once.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_subsample_owner(TreeView t, u32 group_end, float radius, const u32* __restrict__ state,
                                                                         u32* __restrict__ owner)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool valid = p < t.n;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    u32 mine = DROPPED;
    if (valid) {
        c = lane_query<true>(t, QueryView{}, p);
        mine = state[p];
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const bool search = valid && mine != KEPT;
    float bound = search ? radius * radius : -1.f;
    u64 best = ~0ull;
    if (any_lane(search)) {
        auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= bound; };
        walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
            const Leaf lf = load_const(record);
            const States8 st = load_const(reinterpret_cast<const States8*>(state + static_cast<u64>(leaf) * LEAF));
#pragma unroll
            for (int j = 0; j < LEAF; ++j) {
                if (st.v[j] != KEPT) continue;  // (wave-uniform)
                const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
                const float d2 = sq3(dx, dy, dz);
                if (d2 <= bound) {  // (an idle lane: bound = -1)
                    const u64 cand = (static_cast<u64>(__float_as_uint(d2)) << 32) | lf.id[j];
                    best = cand < best ? cand : best;
                    bound = d2 < bound ? d2 : bound;
                }
            }
        });
    }
    if (valid) owner[c.row] = search ? static_cast<u32>(best) : c.row;
}

// the keep mask by input row (the rows of points outside the grid were cleared before)
__global__ __launch_bounds__(SS_BLOCK) void k_subsample_rows(TreeView t, const u32* __restrict__ state, uint8_t* __restrict__ keep)
{
    const u32 p = blockIdx.x * SS_BLOCK + threadIdx.x;
    if (p >= t.n) return;
    keep[t.leaves[p / LEAF].id[p % LEAF]] = state[p] == KEPT ? 1 : 0;
}

int check_subsample_args(const char* what, float radius, u32 flags, const void* keep)
{
    if (const int st = check_radius(what, radius)) return st;
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

}  // namespace

// On the handle's stream, which is synchronised after every ROUND_BATCH rounds (the host reads the decided counter); what follows
// the last round is only enqueued.  Scratch of the handle: the state words (one per leaf slot, and room for one word per input row:
// the scan's places, once the states have gone to the rows), the scan's tile sums and the counter.
int subsample_self(Index& ix, float radius, u32 seed, uint8_t* d_keep, u32* d_owner, u32* d_kept_rows, u64* d_kept_count, u32* rounds_out)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    u32 rounds = 0;
    if (rounds_out) *rounds_out = 0;
    if (rows == 0) {
        if (d_kept_count) PCPX_HIP(hipMemsetAsync(d_kept_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    const u64 npos = static_cast<u64>(ix.nleaves) * LEAF;  // >= n
    const u32 ntiles = scan_tiles(rows);
    Carve c;
    const size_t state_at = c.take((npos > rows ? npos : rows) * sizeof(u32)), sums_at = c.take((ntiles + 1ull) * sizeof(u32)),
                 decided_at = c.take(sizeof(u32));
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    u32* state = reinterpret_cast<u32*>(base + state_at);
    u32* sums = reinterpret_cast<u32*>(base + sums_at);
    u32* decided = reinterpret_cast<u32*>(base + decided_at);
    if (n != rows) {  // the rows of the points outside the voxel grid: dropped, no owner
        PCPX_HIP(hipMemsetAsync(d_keep, 0, rows * sizeof(uint8_t), s));
        if (d_owner) PCPX_HIP(hipMemsetAsync(d_owner, 0xFF, rows * sizeof(u32), s));
    }
    if (n > 0) {
        const TreeView t = ix.view();
        const u64 groups = (n + GROUP - 1) / GROUP;
        const u32 grid = grid_for_groups(groups);
        ProfileScope prof(ix, PCPX_K_RANGE);
        PCPX_HIP(hipMemsetAsync(decided, 0, sizeof(u32), s));
        k_subsample_init<<<blocks_of(npos, SS_BLOCK), SS_BLOCK, 0, s>>>(static_cast<u32>(n), static_cast<u32>(npos), state);
        for (u32 so_far = 0; so_far < n;) {
            for (u32 b = 0; b < ROUND_BATCH; ++b, ++rounds)
                k_subsample_round<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, seed, state, decided);
            if (rounds_out) *rounds_out = rounds;  // (also what an error return below reports)
            PCPX_HIP(hipGetLastError());
            u32 now = 0;
            PCPX_HIP(hipMemcpyAsync(&now, decided, sizeof(u32), hipMemcpyDeviceToHost, s));
            PCPX_HIP(hipStreamSynchronize(s));
            if (now <= so_far || now > n) {  // (every round decides the undecided point of smallest key: this is a fault, not data)
                set_error("pcpx: subsample round %u decided %u of %llu points after %u", rounds, now, static_cast<unsigned long long>(n), so_far);
                return PCPX_ERR_DEVICE;
            }
            so_far = now;
        }
        if (d_owner) k_subsample_owner<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, state, d_owner);
        k_subsample_rows<<<blocks_of(n, SS_BLOCK), SS_BLOCK, 0, s>>>(t, state, d_keep);
        PCPX_HIP(hipGetLastError());
    }
    // (the state words are free by now: the scan's places)
    return count_and_compact_kept(d_keep, rows, state, sums, d_kept_rows, d_kept_count, s);
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_subsample_self_dev(pcpx_index* h, float radius, uint32_t seed, uint32_t flags, uint8_t* d_keep, uint32_t* d_opt_owner,
                            uint32_t* d_opt_kept_rows, uint64_t* d_opt_kept_count, uint32_t* opt_rounds)
{
    static const char* what = "pcpx_subsample_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_subsample_args(what, radius, flags, d_keep)) != PCPX_OK) return st;
        return subsample_self(*ix, radius, seed, d_keep, d_opt_owner, d_opt_kept_rows, d_opt_kept_count, opt_rounds);
    });
}

int pcpx_subsample_self(pcpx_index* h, float radius, uint32_t seed, uint32_t flags, uint8_t* keep, uint32_t* opt_owner,
                        uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint32_t* opt_rounds)
{
    static const char* what = "pcpx_subsample_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_subsample_args(what, radius, flags, keep)) != PCPX_OK) return st;
        if (opt_kept_count) *opt_kept_count = 0;
        if (opt_rounds) *opt_rounds = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        uint8_t* dk = stage.alloc<uint8_t>(rows * sizeof(uint8_t));
        u32* dw = stage.alloc_for(opt_owner, rows * sizeof(u32));
        u32* dr = stage.alloc_for(opt_kept_rows, rows * sizeof(u32));
        u64* dt = opt_kept_rows || opt_kept_count ? stage.alloc<u64>(sizeof(u64)) : nullptr;
        if ((st = stage.st) != PCPX_OK || (st = subsample_self(*ix, radius, seed, dk, dw, dr, dt, opt_rounds)) != PCPX_OK) return st;
        stage.download(keep, dk, rows * sizeof(uint8_t));
        stage.download_opt(opt_owner, dw, rows * sizeof(u32));
        return download_kept(stage, dt, dr, opt_kept_count, opt_kept_rows);
    });
}

}  // extern "C"
