// pcpx_fps.hip -- farthest point sampling of the indexed cloud (include/pcpx_fps.h).
//
// A BUCKET is the set of leaf slots under one tree node of height H (H = 2: 16 leaf records, 128 slots); its box is that node's
// NodeBox, tight over its points.  The state, in the handle's scratch: one float D per leaf slot, one owner ordinal per slot when
// owners are asked for, one 64-bit KEY per bucket and the WINNER of each sample (below).  A key is
//     bits(D) << 32 | (0xFFFFFFFF - input index)
// of the slot with the largest D, the lowest input index among equals: D is never negative, so its bits order as the float does
// (+inf included), and the larger key is the contract's next sample.  Key 0: nothing here (no indexed row is 0xFFFFFFFF).
//
// One launch per sample t, one wave per 64 buckets, one lane per bucket.  The buckets are dealt to the waves like cards: lane l of
// wave w of W stands for bucket l W + w, so the buckets round a sample -- neighbours on the curve, and the only ones it updates --
// belong to as many different waves as there are.  (With wave w on the buckets 64 w .. 64 w + 63 a few waves updated all of a
// sample's buckets one after the other while the others had none: 74 against 18 us per sample at 10 M points)
// The keys lie in the waves' order, key[64 w + l], and so do copies of the boxes, bound by bound, so a wave reads its own 64 as
// whole pieces.  (The copies changed no time against 32-byte reads from the tree at a stride of W boxes: section 32.)
//
// A wave reads winner[t], which the launch before it left (the kernel boundary is the hand-off); 0, or a distance within the stop
// radius, and it returns -- the launches after it then find winner[t + 1] == 0 and return as well: that cascade is the whole stop
// rule, on the device.  Else lane l
// needs its bucket iff box_d2(box_b, s) < max_b: box_d2 (pcpx_device.h, unfused) is in float a lower bound of every contained
// point's d2 (pcpx_box_bound.h), so in a bucket skipped under >= no d2 is below any D: nothing would change.  The wave then updates
// the needed buckets one after the other, all 64 lanes on one bucket's slots, reduces the bucket's new key and stores it from one
// lane; at the end one agent-scope 64-bit atomic maximum per wave into winner[t + 1], over the keys of all its buckets, updated or
// not.  The maximum commutes, a bucket is only ever touched by its own wave, and nothing else crosses workgroups inside a launch.
//
// THE WINNER of sample t is the maximum of WIN_SLOTS words: wave w adds to word w % WIN_SLOTS, and every wave of the next launch
// reads all of them (one lane each) and takes their maximum.  (Into ONE word the atomics of a launch stand in line: 12 ns each,
// 59 us per sample for the 4900 waves of 10 M points at height 1; section 32.)  The words of three samples are a ring: launch t
// reads entry t % 3, adds to entry (t + 1) % 3 and clears entry (t + 2) % 3, which launch t - 1 read and launch t + 1 adds to.
// So the state does not grow with m, and nothing but the ring's 1.5 KB is cleared per call.
#include "pcpx_device.h"
#include "pcpx_fps.h"
#include "pcpx_stage.h"

namespace pcpx {

namespace {

constexpr u32 FPS_WAVES = 4;  // waves per block of the bucket kernels
constexpr u32 FPS_BLOCK = 64 * FPS_WAVES;
// the default bucket height (measured: DESIGN.md section 32): 1 up to this many leaves -- 2^18 points --, 2 beyond
constexpr u32 FPS_HEIGHT_1_LEAVES = 1u << 15;
constexpr u32 INF_BITS = 0x7F800000u;
constexpr u32 WIN_SLOTS = 64, WIN_RING = 3;  // (below: the winner)
constexpr u32 ONE_BLOCK_SLOTS = 8u * 1024u;  // the most leaf slots the one-block form holds
constexpr u32 ONE_BLOCK_BELOW = 8u * 1024u;  // ... and the most for which it is used by default (measured: DESIGN.md section 32)

struct FpsState {
    float* D;     // per leaf slot
    u32* owner;   // per leaf slot, or null
    u64* key;     // per bucket, in the waves' order: 64 per wave
    u64* winner;  // WIN_RING entries of WIN_SLOTS keys: sample t's is the maximum of entry t % WIN_RING
    float* box;   // the buckets' boxes in the waves' order, one array per bound: lo x, y, z, hi x, y, z, `stride` floats each
    u32 stride;   // 64 * waves
};

__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ u64 key_of(const float d, const u32 id) { return (static_cast<u64>(__float_as_uint(d)) << 32) | (~id); }

// All 64 lanes on bucket b: slot s of it is taken by lane s & 63, so the lanes 8 j .. 8 j + 7 read the eight x of one leaf record
// side by side.  INIT: D = +inf (0 for a slot that holds no point: it never wins), no owner; a slot that holds row `start` puts
// its key into winner[0].  Else: the sample (sx, sy, sz), ordinal t.  Returns the bucket's key, in every lane.
template <int H, bool INIT>
__device__ __forceinline__ u64 bucket_pass(const TreeView& t, const u32 b, const u32 lane, const FpsState& st, const float sx, const float sy,
                                           const float sz, const u32 ordinal, const u32 start)
{
    constexpr u32 S = static_cast<u32>(LEAF) << (2 * H);  // slots of a bucket
    constexpr u32 PER_LANE = S > 64u ? S / 64u : 1u;
    const u64 nslots = static_cast<u64>(t.nleaves) * LEAF;
    u64 key = 0;
#pragma unroll
    for (u32 u = 0; u < PER_LANE; ++u) {
        const u32 s = u * 64u + lane;
        const u64 slot = static_cast<u64>(b) * S + s;
        if (s < S && slot < nslots) {
            const Leaf& lf = t.leaves[slot / LEAF];
            const u32 j = static_cast<u32>(slot % LEAF);
            const u32 id = lf.id[j];
            const bool real = id != INVALID_ID;
            float d;
            if (INIT) {
                d = real ? __uint_as_float(INF_BITS) : 0.f;
                st.D[slot] = d;
                if (st.owner) st.owner[slot] = PCPX_FPS_NONE;
                if (real && id == start) __hip_atomic_fetch_max(st.winner, key_of(d, id), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (entry 0, slot 0)
            } else {
                const float dx = lf.x[j] - sx, dy = lf.y[j] - sy, dz = lf.z[j] - sz;
                const float now = sq3(dx, dy, dz);  // (NaN in a slot that holds no point: the compare fails)
                d = st.D[slot];
                if (now < d) {
                    d = now;
                    st.D[slot] = now;
                    if (st.owner) st.owner[slot] = ordinal;
                }
            }
            const u64 mine = real ? key_of(d, id) : 0ull;
            key = mine > key ? mine : key;
        }
    }
    return wave_max(key);
}

// the slots of bucket b that lie in a leaf record: what a pass over it evaluates
template <int H>
__device__ __forceinline__ u32 bucket_slots(const TreeView& t, const u32 b)
{
    constexpr u64 S = static_cast<u64>(LEAF) << (2 * H);
    const u64 nslots = static_cast<u64>(t.nleaves) * LEAF, first = b * S;
    return static_cast<u32>(nslots - first < S ? nslots - first : S);
}

// (level_first: the heap id of the first node of the buckets' tree level.)  Every D, owner, bucket key and box, and winner[0]: the key of row `start` if a slot holds it, or with PCPX_FPS_START_LOWEST the
// largest bucket key -- every D is +inf, so that is the lowest indexed row.
template <int H>
__global__ __launch_bounds__(FPS_BLOCK) void k_fps_init(TreeView t, u32 nbuckets, u32 nwaves, u32 level_first, FpsState st, u32 start)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 w = blockIdx.x * FPS_WAVES + wave_in_block();
    if (w >= nwaves) return;
    if (lane * nwaves + w < nbuckets) {  // this lane's box, from the tree to where the wave reads its 64 as six pieces
        const NodeBox nb = t.nodes[level_first + lane * nwaves + w];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            st.box[a * st.stride + w * 64u + lane] = nb.lo(a);
            st.box[(3 + a) * st.stride + w * 64u + lane] = nb.hi(a);
        }
    }
    u64 best = 0;
    for (u32 i = 0; i < 64u; ++i) {
        const u32 b = i * nwaves + w;  // (wave-uniform; ascending in i)
        if (b >= nbuckets) break;
        const u64 key = bucket_pass<H, true>(t, b, lane, st, 0.f, 0.f, 0.f, 0u, start);
        if (lane == 0) st.key[w * 64u + i] = key;
        best = key > best ? key : best;
    }
    if (start == PCPX_FPS_START_LOWEST && lane == 0 && best != 0ull)
        __hip_atomic_fetch_max(st.winner + (w % WIN_SLOTS), best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (entry 0)
}

struct FpsOut {
    u32* rows;
    float* d2;
    u64* count;
    u64* evaluations;
};

// sample `ordinal` (see the head of the file)
template <int H>
__global__ __launch_bounds__(FPS_BLOCK) void k_fps_sample(TreeView t, u32 nbuckets, u32 nwaves, FpsState st,
                                                         const float* __restrict__ xyz, u32 ordinal, u32 stop_bits, u32 prune, FpsOut out)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 w = blockIdx.x * FPS_WAVES + wave_in_block();
    if (w >= nwaves) return;
    // entry (t + 2) % WIN_RING, which the launch before this one read, is cleared for the launch after this one -- before the test
    // below, so that once a launch has returned there every later one finds zeros
    if (w == 0u) __hip_atomic_store(st.winner + ((ordinal + 2u) % WIN_RING) * WIN_SLOTS + lane, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 win = wave_max(__hip_atomic_load(st.winner + (ordinal % WIN_RING) * WIN_SLOTS + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const u32 win_bits = static_cast<u32>(win >> 32);
    if (win == 0ull || (ordinal != 0u && win_bits <= stop_bits)) return;  // (wave-uniform, and the same in every wave)
    const u32 row = ~static_cast<u32>(win);
    if (w == 0u && lane == 0u) {
        out.rows[ordinal] = row;
        if (out.d2) out.d2[ordinal] = __uint_as_float(win_bits);
        *out.count = static_cast<u64>(ordinal) + 1ull;
    }
    const float sx = xyz[3ull * row], sy = xyz[3ull * row + 1], sz = xyz[3ull * row + 2];
    const u32 b = lane * nwaves + w;
    u64 mine = 0;
    bool need = false;
    if (b < nbuckets) {
        mine = st.key[w * 64u + lane];
        const float* at = st.box + w * 64u + lane;
        NodeBox box;
        box.set(at[0], at[st.stride], at[2ull * st.stride], at[3ull * st.stride], at[4ull * st.stride], at[5ull * st.stride]);
        box.poison = 0.f;  // (a real node's)
        box.pad = 0.f;
        // (a real node: poison +0.  The test fails for a NaN, and for +inf against +inf, where no d2 can be below D either)
        need = prune == 0u || box_d2(box, sx, sy, sz) < __uint_as_float(static_cast<u32>(mine >> 32));
    }
    u64 todo = __builtin_amdgcn_ballot_w64(need);
    u32 evaluated = 0;
    while (todo != 0ull) {
        const u32 i = static_cast<u32>(__builtin_ctzll(todo));
        todo &= todo - 1ull;
        const u32 bb = i * nwaves + w;
        const u64 key = bucket_pass<H, false>(t, bb, lane, st, sx, sy, sz, ordinal, 0u);
        evaluated += bucket_slots<H>(t, bb);
        if (lane == i) {
            mine = key;
            st.key[w * 64u + lane] = key;
        }
    }
    const u64 best = wave_max(mine);
    if (lane == 0u) {
        if (best != 0ull)
            __hip_atomic_fetch_max(st.winner + ((ordinal + 1u) % WIN_RING) * WIN_SLOTS + (w % WIN_SLOTS), best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (out.evaluations && evaluated != 0u)
            __hip_atomic_fetch_add(out.evaluations, static_cast<u64>(evaluated), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// D and the owner from the slots to the input rows (the rows of the points outside the grid were filled before)
__global__ __launch_bounds__(FPS_BLOCK) void k_fps_rows(TreeView t, FpsState st, float* __restrict__ min_d2, u32* __restrict__ owner)
{
    const u32 p = blockIdx.x * FPS_BLOCK + threadIdx.x;
    if (p >= t.n) return;
    const u32 row = t.leaves[p / LEAF].id[p % LEAF];
    if (min_d2) min_d2[row] = st.D[p];
    if (owner) owner[row] = st.owner[p];
}

// ---- small clouds: the whole loop in ONE launch of ONE workgroup ----------------------------------------------------------------------------
// A cloud of up to ONE_THREADS * ONE_PER leaf slots lives in the registers of one workgroup: thread i holds the slots u * ONE_THREADS + i
// with x, y, z, D, the input index and (OWNER) the owner ordinal.  A sample is one pass over the registers, a wave-wide maximum of the
// keys, one LDS word per wave and ONE barrier: every thread then takes the maximum of the waves' words itself (the words alternate
// between two sets, so a wave that runs ahead by one sample writes the other set, and it cannot run ahead by two: the barrier
// between lies behind the slowest wave's reads).  No pruning -- every sample looks at every slot -- and no launch per sample: the
// same keys, the same maximum, the same bits.  (Sixteen slots a thread do not fit: a workgroup of 1024 threads has 128 registers a
// thread, and hipcc spilled 128 to 258 of them.)
constexpr u32 ONE_THREADS = 1024, ONE_WAVES = ONE_THREADS / 64;
constexpr int ONE_PER = 8;
static_assert(ONE_THREADS * ONE_PER == ONE_BLOCK_SLOTS, "the one-block form's limit");

template <int PER, bool OWNER>
__global__ __launch_bounds__(ONE_THREADS) void k_fps_one_block(TreeView t, const float* __restrict__ xyz, u32 launches, u32 start, u32 stop_bits,
                                                               FpsOut out, float* __restrict__ min_d2, u32* __restrict__ owner)
{
    __shared__ u64 wave_key[2][ONE_WAVES];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const u32 nslots = t.nleaves * LEAF;
    float x[PER], y[PER], z[PER], D[PER];
    u32 id[PER], own[OWNER ? PER : 1];
    u64 key = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const u32 slot = u * ONE_THREADS + threadIdx.x;
        x[u] = y[u] = z[u] = D[u] = 0.f;
        id[u] = INVALID_ID;
        if (OWNER) own[u] = PCPX_FPS_NONE;
        if (slot < nslots) {
            const Leaf& lf = t.leaves[slot / LEAF];
            x[u] = lf.x[slot % LEAF], y[u] = lf.y[slot % LEAF], z[u] = lf.z[slot % LEAF], id[u] = lf.id[slot % LEAF];
        }
        if (id[u] != INVALID_ID) {
            D[u] = __uint_as_float(INF_BITS);
            const u64 mine = key_of(D[u], id[u]);
            if (start == PCPX_FPS_START_LOWEST || id[u] == start) key = mine > key ? mine : key;
        }
    }
    u32 taken = 0;
    for (u32 ordinal = 0;; ++ordinal) {
        // the block's maximum of `key`: the sample this trip takes
        key = wave_max(key);
        if (lane == 0) wave_key[ordinal & 1u][w] = key;
        __syncthreads();
        u64 win = 0;
#pragma unroll
        for (u32 i = 0; i < ONE_WAVES; ++i) {
            const u64 k = wave_key[ordinal & 1u][i];
            win = k > win ? k : win;
        }
        const u32 win_bits = static_cast<u32>(win >> 32);
        if (ordinal == launches || win == 0ull || (ordinal != 0u && win_bits <= stop_bits)) break;  // (block-uniform)
        const u32 row = ~static_cast<u32>(win);
        if (threadIdx.x == 0) {
            out.rows[ordinal] = row;
            if (out.d2) out.d2[ordinal] = __uint_as_float(win_bits);
        }
        taken = ordinal + 1u;
        const float sx = xyz[3ull * row], sy = xyz[3ull * row + 1], sz = xyz[3ull * row + 2];
        key = 0;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const float dx = x[u] - sx, dy = y[u] - sy, dz = z[u] - sz;
            const float now = sq3(dx, dy, dz);
            if (now < D[u]) {  // (a slot that holds no point: D = 0, and no d2 is below it)
                D[u] = now;
                if (OWNER) own[u] = ordinal;
            }
            const u64 mine = id[u] != INVALID_ID ? key_of(D[u], id[u]) : 0ull;
            key = mine > key ? mine : key;
        }
    }
    if (threadIdx.x == 0) {
        *out.count = taken;
        if (out.evaluations) *out.evaluations = static_cast<u64>(taken) * nslots;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (id[u] == INVALID_ID) continue;
        if (min_d2) min_d2[id[u]] = D[u];
        if (OWNER) owner[id[u]] = own[u];
    }
}

template <int PER>
void launch_one_block(Index& ix, u32 launches, u32 start, u32 stop_bits, const FpsOut& out, float* d_min_d2, u32* d_owner)
{
    if (d_owner) k_fps_one_block<PER, true><<<1, ONE_THREADS, 0, ix.stream>>>(ix.view(), ix.d_xyz, launches, start, stop_bits, out, d_min_d2, d_owner);
    else k_fps_one_block<PER, false><<<1, ONE_THREADS, 0, ix.stream>>>(ix.view(), ix.d_xyz, launches, start, stop_bits, out, d_min_d2, d_owner);
}

int check_fps(const char* what, u64 m, const pcpx_fps_params* p, const void* rows, const void* count)
{
    if (!p) {
        set_error("%s: params is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (p->flags & ~PCPX_FPS_ON_DEVICE) {
        set_error("%s: unknown flag bits 0x%x", what, p->flags);
        return PCPX_ERR_INVALID;
    }
    if (p->reserved != 0u) {
        set_error("%s: params->reserved must be 0", what);
        return PCPX_ERR_INVALID;
    }
    if (const int st = check_radius(what, p->stop_radius)) return st;
    if (!count) {
        set_error("%s: out_count is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (m > 0 && !rows) {
        set_error("%s: out_rows is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

// (needs the handle: after the argument checks, still before any device call)
int check_fps_start(const char* what, const Index& ix, const pcpx_fps_params& p)
{
    if (p.start == PCPX_FPS_START_LOWEST || p.start < ix.n_in) return PCPX_OK;
    set_error("%s: start is row %u of %llu", what, p.start, static_cast<unsigned long long>(ix.n_in));
    return PCPX_ERR_INVALID;
}

template <int H>
int launch_fps(Index& ix, const FpsState& st, u32 launches, u32 start, u32 stop_bits, const FpsOut& out)
{
    hipStream_t s = ix.stream;
    const TreeView t = ix.view();
    const u32 nbuckets = static_cast<u32>((static_cast<u64>(t.nleaves) + (1ull << (2 * H)) - 1ull) >> (2 * H));
    const u32 level_first = static_cast<u32>(((1ull << (2 * (t.depth - H))) - 1ull) / 3ull);
    const u32 nwaves = blocks_of(nbuckets, 64u), grid = blocks_of(nwaves, FPS_WAVES);
    const u32 prune = ix.tuning.fps_prune ? 1u : 0u;
    k_fps_init<H><<<grid, FPS_BLOCK, 0, s>>>(t, nbuckets, nwaves, level_first, st, start);
    for (u32 ordinal = 0; ordinal < launches; ++ordinal)
        k_fps_sample<H><<<grid, FPS_BLOCK, 0, s>>>(t, nbuckets, nwaves, st, ix.d_xyz, ordinal, stop_bits, prune, out);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

// Everything is enqueued on the handle's stream; nothing is read back.  The scratch is the handle's, one Carve ensured once before
// the first launch; every word of it that is read was written by this call.
int fps_self(Index& ix, u64 m, const pcpx_fps_params& p, u32* d_rows, u64* d_count, float* d_d2, float* d_min_d2, u32* d_owner, u64* d_evaluations)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    PCPX_HIP(hipMemsetAsync(d_count, 0, sizeof(u64), s));
    if (d_evaluations) PCPX_HIP(hipMemsetAsync(d_evaluations, 0, sizeof(u64), s));
    if (rows == 0) return PCPX_OK;
    const bool selects = n > 0 && m > 0;
    if (!selects || n != rows) {  // the rows that no slot holds (all of them when nothing is selected)
        if (d_min_d2 && (st = launch_fill_f32(d_min_d2, rows, std::numeric_limits<float>::infinity(), s)) != PCPX_OK) return st;
        if (d_owner) PCPX_HIP(hipMemsetAsync(d_owner, 0xFF, rows * sizeof(u32), s));
    }
    if (!selects) return PCPX_OK;
    if (!ix.d_xyz) {
        set_error("pcpx_farthest_points_self: the handle keeps no copy of its cloud");
        return PCPX_ERR_UNSUPPORTED;
    }
    const u64 nslots = static_cast<u64>(ix.nleaves) * LEAF;
    const u32 launches = static_cast<u32>(m < n ? m : n);
    const FpsOut out{d_rows, d_d2, d_count, d_evaluations};
    const float stop2 = p.stop_radius * p.stop_radius;
    u32 stop_bits;
    std::memcpy(&stop_bits, &stop2, sizeof(stop_bits));
    const bool fits = nslots <= ONE_BLOCK_SLOTS;
    if (ix.tuning.fps_one_block < 0 ? nslots <= ONE_BLOCK_BELOW : (ix.tuning.fps_one_block != 0 && fits)) {
        launch_one_block<ONE_PER>(ix, launches, p.start, stop_bits, out, d_min_d2, d_owner);
        PCPX_HIP(hipGetLastError());
        return PCPX_OK;
    }
    // a tree of depth 0 is one leaf, its own bucket; the others have depth >= 2
    const int wanted = ix.tuning.fps_bucket_height ? ix.tuning.fps_bucket_height : ix.nleaves <= FPS_HEIGHT_1_LEAVES ? 1 : 2;
    const int height = wanted < ix.depth ? wanted : ix.depth;
    const u64 nbuckets = (static_cast<u64>(ix.nleaves) + (1ull << (2 * height)) - 1ull) >> (2 * height);
    const u64 stride = (nbuckets + 63ull) / 64ull * 64ull;  // 64 entries per wave
    Carve c;
    const size_t d_at = c.take(nslots * sizeof(float)), owner_at = d_owner ? c.take(nslots * sizeof(u32)) : 0,
                 key_at = c.take(stride * sizeof(u64)), box_at = c.take(6ull * stride * sizeof(float)), winner_at = c.take(WIN_RING * WIN_SLOTS * sizeof(u64));
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    FpsState state;
    state.D = reinterpret_cast<float*>(base + d_at);
    state.owner = d_owner ? reinterpret_cast<u32*>(base + owner_at) : nullptr;
    state.key = reinterpret_cast<u64*>(base + key_at);
    state.winner = reinterpret_cast<u64*>(base + winner_at);
    state.box = reinterpret_cast<float*>(base + box_at);
    state.stride = static_cast<u32>(stride);
    PCPX_HIP(hipMemsetAsync(state.winner, 0, WIN_RING * WIN_SLOTS * sizeof(u64), s));
    switch (height) {
    case 0: st = launch_fps<0>(ix, state, launches, p.start, stop_bits, out); break;
    case 1: st = launch_fps<1>(ix, state, launches, p.start, stop_bits, out); break;
    case 2: st = launch_fps<2>(ix, state, launches, p.start, stop_bits, out); break;
    default: st = launch_fps<3>(ix, state, launches, p.start, stop_bits, out); break;
    }
    if (st != PCPX_OK) return st;
    if (d_min_d2 || d_owner) {
        k_fps_rows<<<blocks_of(n, FPS_BLOCK), FPS_BLOCK, 0, s>>>(ix.view(), state, d_min_d2, d_owner);
        PCPX_HIP(hipGetLastError());
    }
    return PCPX_OK;
}

// One interval of the PCPX_K_RANGE family for the whole call.
int booked_as_one_range_interval(Index& ix, u64 m, const pcpx_fps_params& p, u32* d_rows, u64* d_count, float* d_d2, float* d_min_d2, u32* d_owner,
                                 u64* d_evaluations)
{
    ProfileScope prof(ix, PCPX_K_RANGE);
    const bool profiling = ix.profiling;
    ix.profiling = false;
    const int st = fps_self(ix, m, p, d_rows, d_count, d_d2, d_min_d2, d_owner, d_evaluations);
    ix.profiling = profiling;
    return st;
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_farthest_points_self(pcpx_index* h, uint64_t m, const pcpx_fps_params* params, uint32_t* out_rows, uint64_t* out_count, float* opt_out_d2,
                              float* opt_out_min_d2, uint32_t* opt_out_owner, uint64_t* opt_out_evaluations)
{
    static const char* what = "pcpx_farthest_points_self";
    if (const int st = check_fps(what, m, params, out_rows, out_count)) return st;
    if (params->flags & PCPX_FPS_ON_DEVICE) {
        return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
            if (const int st = check_fps_start(what, *ix, *params)) return st;
            return booked_as_one_range_interval(*ix, m, *params, out_rows, out_count, opt_out_d2, opt_out_min_d2, opt_out_owner,
                                                opt_out_evaluations);
        });
    }
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_fps_start(what, *ix, *params)) != PCPX_OK) return st;
        *out_count = 0;
        if (opt_out_evaluations) *opt_out_evaluations = 0;
        const u64 rows = ix->n_in, most = m < ix->n ? m : ix->n;  // count <= most
        u64* dc = stage.alloc<u64>(sizeof(u64));
        u64* de = stage.alloc_for(opt_out_evaluations, sizeof(u64));
        u32* dr = stage.alloc<u32>(most * sizeof(u32));
        float* dd = stage.alloc_for(opt_out_d2, most * sizeof(float));
        float* dm = stage.alloc_for(opt_out_min_d2, rows * sizeof(float));
        u32* dw = stage.alloc_for(opt_out_owner, rows * sizeof(u32));
        if ((st = stage.st) != PCPX_OK) return st;
        if ((st = booked_as_one_range_interval(*ix, m, *params, dr, dc, dd, dm, dw, de)) != PCPX_OK) return st;
        u64 count = 0;
        stage.download(&count, dc, sizeof(u64));
        stage.download_opt(opt_out_evaluations, de, sizeof(u64));
        if (rows) stage.download_opt(opt_out_min_d2, dm, rows * sizeof(float));
        if (rows) stage.download_opt(opt_out_owner, dw, rows * sizeof(u32));
        if ((st = stage.wait()) != PCPX_OK) return st;
        *out_count = count;
        if (!count) return PCPX_OK;
        stage.download(out_rows, dr, count * sizeof(u32));
        stage.download_opt(opt_out_d2, dd, count * sizeof(float));
        return stage.wait();
    });
}

}  // extern "C"
