// pcpx_objects.hip -- objects from labels (include/pcpx_objects.h): the member rows ordered by (label, row)
// with one stable sort, cut into segments at the label changes, the segments that pass the size filter numbered, and every sum,
// minimum and maximum of a segment formed in the contract's fixed 64-ary tree.  No LDS outside the scan (pcpx_scan.h) and the sort
// (pcpx_sort.hip), no atomics at all, and nothing is handed between workgroups inside a launch.
//   k_obj_member    one thread per row: is it a member
//   pcpx_scan.h     over the member flags: a member's place among the members, and their number m
//   k_obj_keys      word = label << 32 | row at the member's place; the other rows' words, all ones, behind the m members
//   sort_keys_u64   on the upper half (stable: ascending (label, row); the words of all ones stay behind the members)
//   pcpx_scan.h     over the head flags (the label differs from its predecessor's): a position's segment, and their number
//   k_obj_starts    where every segment starts
//   pcpx_scan.h     over the segments, 64-bit: low half 1 for an object, upper half its members -- an object's number and offset, S
//   k_obj_heads / k_obj_rows / k_obj_finish    labels, counts, first rows, offsets; the rows by object and the object of every row
//   k_obj_tree      one lane per chunk per level; three passes: centroid and AABB, covariance, the oriented box's extents
//   k_obj_axes      one thread per object: the Jacobi sweeps of pcpx_horn.h
#include "pcpx_device.h"
#include "pcpx_horn.h"
#include "pcpx_lease.h"
#include "pcpx_objects.h"
#include "pcpx_scan.h"

#include <algorithm>
#include <cmath>

namespace pcpx {

namespace {

constexpr u32 OB_BLOCK = 256;
constexpr u32 OB_CHUNK = PCPX_OBJECTS_CHUNK;  // the tree's fan-in (the contract's)
constexpr int OB_LEVELS = 6;                  // 64^6 = 2^36 members: more than a call can have
constexpr u64 OB_N_LIMIT = (1ull << 32) - SORT_TILE_WORDS;
constexpr u64 OB_FILLER = ~0ull;  // the word of a row that is not a member
constexpr u32 OB_KNOWN_FLAGS = PCPX_OBJECTS_ON_DEVICE | PCPX_OBJECTS_SKIP;

// The words of a call on the device.  total: the objects in its low half, their members in its upper half.
struct State {
    u64 members, segments, total;
};

// What a chunk hands up the tree: six float64 words and six 32-bit ones, of which each pass uses its own.
struct Value {
    double d[6];
    u32 w[6];
};

// (field by field: a copy of the whole struct is an array in memory to the compiler, which then keeps it in LDS)
__device__ __forceinline__ void load_value(const Value* __restrict__ from, Value& x)
{
#pragma unroll
    for (int a = 0; a < 6; ++a) x.d[a] = from->d[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) x.w[a] = from->w[a];
}
__device__ __forceinline__ void store_value(Value* __restrict__ to, const Value& x)
{
#pragma unroll
    for (int a = 0; a < 6; ++a) to->d[a] = x.d[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) to->w[a] = x.w[a];
}

// The chunks of level l hold W = 64^(l + 1) members.  The partial sums of the segments of more than W members live in slots by
// position, one array per level.  Such a segment spans more than W positions, so a window of W aligned positions meets at most two
// of them: three would put the middle one wholly inside the window.  The later of the two starts inside the window, and it is the
// only one that does (one that starts inside reaches past the window's end, so nothing starts behind it); the earlier one started
// before the window.  A segment's chunks start W positions apart, so a window holds at most one chunk start of each.  Hence the
// chunk that starts at position i of a segment that starts at s has slot 2 (i / W) + (s / W == i / W), and no two chunks share
// one: pcpx_voxel.hip's chunk_slot with 64^(l + 1) in place of 64.
__host__ __device__ inline u64 tree_slots(u64 n, u64 W) { return 2 * ((n + W - 1) / W); }
__device__ __forceinline__ u64 tree_slot(u64 i, u64 s, u64 W) { return 2 * (i / W) + ((s / W == i / W) ? 1u : 0u); }
__host__ __device__ inline u64 chunk_members(int level)  // 64^(level + 1)
{
    return 1ull << (6 * (level + 1));
}

struct Layout {
    size_t state = 0, flag = 0, word[2] = {0, 0}, seg = 0, sums = 0, start = 0, slots[OB_LEVELS] = {0, 0, 0, 0, 0, 0}, centroid = 0, cov = 0, sort = 0,
           sort_bytes = 0, bytes = 0;
    int levels = 0;  // the levels a call over n rows launches
    u64 cap = 0;     // the objects the per-object arrays have room for
    Layout(u64 n, u64 capacity) : cap(std::min(capacity, n))
    {
        Carve c;
        state = c.take(sizeof(State));
        flag = c.take(n);
        for (size_t& w : word) w = c.take(n * sizeof(u64));
        seg = c.take(n * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(n)) * sizeof(u64));
        start = c.take((n + 1) * sizeof(u32));
        // level l runs when a segment can have more than 64^l members; its slots hold the sums of the segments of more than 64^(l + 1)
        for (levels = 0; levels < OB_LEVELS && (levels == 0 || n > chunk_members(levels - 1)); ++levels)
            slots[levels] = c.take(tree_slots(n, chunk_members(levels)) * sizeof(Value));
        centroid = c.take(cap * 3 * sizeof(double));
        cov = c.take(cap * 6 * sizeof(double));
        sort_keys_u64(nullptr, sort_bytes, nullptr, nullptr, n, nullptr, 32);
        sort = c.take(sort_bytes);
        bytes = c.bytes();
    }
};

// unsigned integers in the order of the floats they are the bits of (-0 below +0)
__device__ __forceinline__ u32 ordered_of(float f)
{
    const u32 b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of_ordered(u32 o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

struct Filter {
    u32 min_size, max_size;
    __device__ __forceinline__ bool operator()(u32 c) const { return min_size <= c && (max_size == 0u || c <= max_size); }
};

__global__ __launch_bounds__(OB_BLOCK) void k_obj_member(const float* __restrict__ points, const u32* __restrict__ labels, u32 n, u32 skip, u32 none_label,
                                                        unsigned char* __restrict__ flag)
{
    const u32 i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 at = static_cast<u64>(i) * 3;
    const bool finite = std::isfinite(points[at]) && std::isfinite(points[at + 1]) && std::isfinite(points[at + 2]);
    flag[i] = (finite && !(skip && labels[i] == none_label)) ? 1 : 0;
}

struct IsMember {
    const unsigned char* flag;
    __device__ u32 operator()(u32 i) const { return flag[i]; }
};

// place[i]: the members before row i.  A member's word goes to its place, another row's behind the m members, in row order too.
__global__ __launch_bounds__(OB_BLOCK) void k_obj_keys(const u32* __restrict__ labels, const unsigned char* __restrict__ flag, const u32* __restrict__ place,
                                                      u32 n, const State* __restrict__ st, u64* __restrict__ word, u32* __restrict__ out_object_of_row)
{
    const u32 i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 before = place[i];
    if (flag[i]) {
        word[before] = (static_cast<u64>(labels[i]) << 32) | i;
    } else {
        const u64 at = st->members + (i - before);  // (below n: the members and the rows before i that are none)
        if (at < n) word[at] = OB_FILLER;
        if (out_object_of_row) out_object_of_row[i] = PCPX_OBJECTS_NONE;
    }
}

// 1 where a segment starts in the (label, row) order
struct IsHead {
    const u64* sorted;
    const State* st;
    __device__ u32 operator()(u32 p) const
    {
        if (p >= st->members) return 0u;
        return (p == 0 || (sorted[p - 1] >> 32) != (sorted[p] >> 32)) ? 1u : 0u;
    }
};

// seg[p]: the heads before position p on entry, the position's segment on return.  start[v] at the head of v, start[v + 1] behind
// the last member (so start[v + 1] is where segment v ends for every v).
__global__ __launch_bounds__(OB_BLOCK) void k_obj_starts(const u64* __restrict__ sorted, const State* __restrict__ st, u32* seg, u32 n, u32* __restrict__ start)
{
    const u32 p = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (p >= n || p >= st->members) return;
    const u32 head = IsHead{sorted, st}(p);
    const u32 v = seg[p] + head - 1u;
    seg[p] = v;
    if (head) start[v] = p;
    if (p + 1 == st->members) start[v + 1] = p + 1;
}

// a segment's word of the third scan: 1 and its members << 32 for an object, 0 otherwise
struct ObjectWord {
    const u32* start;
    const State* st;
    Filter pass;
    __device__ u64 operator()(u32 v) const
    {
        if (v >= st->segments) return 0ull;
        const u32 c = start[v + 1] - start[v];
        return pass(c) ? ((static_cast<u64>(c) << 32) | 1ull) : 0ull;
    }
};

struct Heads {
    u32 *labels, *counts, *first_row, *offsets;
};

// One thread per segment.  num[v]: the objects before segment v (low half) and their members (upper half).  Object `cap` gets its
// offset too: it is where object cap - 1 ends.
__global__ __launch_bounds__(OB_BLOCK) void k_obj_heads(const u64* __restrict__ sorted, const u32* __restrict__ start, const u64* __restrict__ num,
                                                       const State* __restrict__ st, u32 n, u32 cap, Filter pass, Heads out)
{
    const u32 v = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (v >= n || v >= st->segments) return;
    const u32 s = start[v], c = start[v + 1] - s;
    if (!pass(c)) return;
    const u64 w = num[v];
    const u32 o = static_cast<u32>(w);
    if (o > cap) return;
    if (out.offsets) out.offsets[o] = static_cast<u32>(w >> 32);
    if (o == cap) return;
    const u64 head = sorted[s];
    if (out.labels) out.labels[o] = static_cast<u32>(head >> 32);
    if (out.counts) out.counts[o] = c;
    if (out.first_row) out.first_row[o] = static_cast<u32>(head);
}

// One thread per position: the member's object, and its row at its place among the rows of the objects that have room.
__global__ __launch_bounds__(OB_BLOCK) void k_obj_rows(const u64* __restrict__ sorted, const u32* __restrict__ seg, const u32* __restrict__ start,
                                                      const u64* __restrict__ num, const State* __restrict__ st, u32 n, u32 cap, Filter pass,
                                                      u32* __restrict__ out_rows, u32* __restrict__ out_object_of_row)
{
    const u32 p = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (p >= n || p >= st->members) return;
    const u32 row = static_cast<u32>(sorted[p]);
    const u32 v = seg[p], s = start[v], c = start[v + 1] - s;
    const bool object = pass(c);
    const u64 w = num[v];
    const u32 o = static_cast<u32>(w);
    if (out_object_of_row && row < n) out_object_of_row[row] = object ? o : PCPX_OBJECTS_NONE;
    if (out_rows && object && o < cap) {
        const u64 at = (w >> 32) + (p - s);  // (below the members' number, so below n)
        if (at < n) out_rows[at] = row;
    }
}

__global__ __launch_bounds__(64) void k_obj_finish(const State* __restrict__ st, u64 n, u32 cap, u64* __restrict__ out_count, u32* __restrict__ out_offsets,
                                                  u64* __restrict__ out_skipped)
{
    if (threadIdx.x != 0) return;
    const u64 S = st->total & 0xFFFFFFFFull;
    *out_count = S;
    if (out_offsets && S <= cap) out_offsets[S] = static_cast<u32>(st->total >> 32);  // (S = 0: offsets[0] = 0)
    if (out_skipped) *out_skipped = n - st->members;
}

// ---- the tree ----------------------------------------------------------------------------------------------------------------------------
struct Tree {
    const float* points;
    const u64* sorted;
    const u32 *seg, *start;
    const u64* num;
    const State* st;
    u32 n, cap;
    Filter pass;
};

__device__ __forceinline__ void load_row(const Tree& t, u32 row, double (&p)[3], float (&f)[3])
{
    const u64 at = static_cast<u64>(row < t.n ? row : 0u) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f[a] = t.points[at + a];
        p[a] = static_cast<double>(f[a]);
    }
}

// Pass 1: the sums of the coordinates (d[0 .. 2]) and the ordered integers of their minima and maxima (w[0 .. 5]).
struct CentroidPass {
    double* centroid;  // cap x 3 (an output or scratch)
    float* aabb;       // cap x 6, or null
    struct Ctx {};
    __device__ __forceinline__ Ctx begin(u32) const { return Ctx{}; }
    __device__ __forceinline__ void leaf(const Tree& t, const Ctx&, u32 row, Value& x) const
    {
        double p[3];
        float f[3];
        load_row(t, row, p, f);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x.d[a] = p[a];
            x.d[3 + a] = 0.0;
            x.w[a] = x.w[3 + a] = ordered_of(f[a]);
        }
    }
    __device__ __forceinline__ static void merge(Value& acc, const Value& x)
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc.d[a] = acc.d[a] + x.d[a];
            acc.w[a] = min(acc.w[a], x.w[a]);
            acc.w[3 + a] = max(acc.w[3 + a], x.w[3 + a]);
        }
    }
    __device__ __forceinline__ void finish(u32 o, u32 c, const Value& total) const
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) centroid[static_cast<u64>(o) * 3 + a] = total.d[a] / static_cast<double>(c);
        if (aabb) {
#pragma unroll
            for (int a = 0; a < 6; ++a) aabb[static_cast<u64>(o) * 6 + a] = float_of_ordered(total.w[a]);
        }
    }
};

// Pass 2: the six products of the differences from the centroid.
struct CovariancePass {
    const double* centroid;
    double* cov;  // cap x 6 (an output or scratch)
    struct Ctx {
        double m[3];
    };
    __device__ __forceinline__ Ctx begin(u32 o) const
    {
        Ctx c;
#pragma unroll
        for (int a = 0; a < 3; ++a) c.m[a] = centroid[static_cast<u64>(o) * 3 + a];
        return c;
    }
    __device__ __forceinline__ void leaf(const Tree& t, const Ctx& c, u32 row, Value& x) const
    {
        double p[3];
        float f[3];
        load_row(t, row, p, f);
        const double dx = p[0] - c.m[0], dy = p[1] - c.m[1], dz = p[2] - c.m[2];
        x.d[0] = dx * dx, x.d[1] = dx * dy, x.d[2] = dx * dz, x.d[3] = dy * dy, x.d[4] = dy * dz, x.d[5] = dz * dz;
#pragma unroll
        for (int a = 0; a < 6; ++a) x.w[a] = 0u;
    }
    __device__ __forceinline__ static void merge(Value& acc, const Value& x)
    {
#pragma unroll
        for (int a = 0; a < 6; ++a) acc.d[a] = acc.d[a] + x.d[a];
    }
    __device__ __forceinline__ void finish(u32 o, u32 c, const Value& total) const
    {
#pragma unroll
        for (int a = 0; a < 6; ++a) cov[static_cast<u64>(o) * 6 + a] = total.d[a] / static_cast<double>(c);
    }
};

// Pass 3: the extents along the axes that k_obj_axes left in the object's 15 doubles: minima d[0 .. 2], maxima d[3 .. 5].
struct ExtentPass {
    const double* centroid;
    double* obb;  // cap x 15
    struct Ctx {
        double m[3], e[9];
    };
    __device__ __forceinline__ Ctx begin(u32 o) const
    {
        Ctx c;
#pragma unroll
        for (int a = 0; a < 3; ++a) c.m[a] = centroid[static_cast<u64>(o) * 3 + a];
#pragma unroll
        for (int a = 0; a < 9; ++a) c.e[a] = obb[static_cast<u64>(o) * 15 + 3 + a];
        return c;
    }
    __device__ __forceinline__ void leaf(const Tree& t, const Ctx& c, u32 row, Value& x) const
    {
        double p[3];
        float f[3];
        load_row(t, row, p, f);
        const double dx = p[0] - c.m[0], dy = p[1] - c.m[1], dz = p[2] - c.m[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double tk = ((dx * c.e[3 * k] + dy * c.e[3 * k + 1]) + dz * c.e[3 * k + 2]) + 0.0;  // (a zero is +0)
            x.d[k] = x.d[3 + k] = tk;
            x.w[k] = x.w[3 + k] = 0u;
        }
    }
    __device__ __forceinline__ static void merge(Value& acc, const Value& x)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc.d[k] = x.d[k] < acc.d[k] ? x.d[k] : acc.d[k];
            acc.d[3 + k] = x.d[3 + k] > acc.d[3 + k] ? x.d[3 + k] : acc.d[3 + k];
        }
    }
    __device__ __forceinline__ void finish(u32 o, u32, const Value& total) const
    {
        double* out = obb + static_cast<u64>(o) * 15;
        double centre[3] = {centroid[static_cast<u64>(o) * 3], centroid[static_cast<u64>(o) * 3 + 1], centroid[static_cast<u64>(o) * 3 + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double mid = (total.d[k] + total.d[3 + k]) / 2.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) centre[a] = centre[a] + mid * out[3 + 3 * k + a];
            out[12 + k] = (total.d[3 + k] - total.d[k]) / 2.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = centre[a];
    }
};

// One lane per chunk of level `level`: Wl = 64^level members per term, W = 64 Wl per chunk.  Threads [0, firsts) take a segment's
// first chunk: at level 0 thread v takes segment v; above, thread k takes the one segment of more than Wl members that starts in
// window k of Wl positions -- it covers the window's last position.  Threads from `firsts` on take the later chunks: thread
// firsts + k the chunk in window k of W positions of the segment that reaches into that window from before it.  A segment of at
// most W members is finished here; a longer one's chunk sums go to their slots.  (Levels above 0 see only segments of more than Wl
// members: the others were finished below.)
template <class Pass>
__global__ __launch_bounds__(OB_BLOCK) void k_obj_tree(Tree t, int level, u64 firsts, Pass pass, const Value* __restrict__ lower, Value* __restrict__ upper)
{
    const u64 id = static_cast<u64>(blockIdx.x) * OB_BLOCK + threadIdx.x;
    const u64 Wl = level == 0 ? 1ull : chunk_members(level - 1), W = chunk_members(level), m = t.st->members;
    u32 v;
    u64 s, i;
    if (id < firsts) {
        if (level == 0) {
            if (id >= t.st->segments) return;
            v = static_cast<u32>(id);
            s = t.start[v];
        } else {
            const u64 last = (id + 1) * Wl - 1;
            if (last >= m) return;
            v = t.seg[last];
            s = t.start[v];
            if (s < id * Wl) return;
        }
        i = s;
    } else {
        const u64 p = (id - firsts) * W;
        if (p >= m) return;
        v = t.seg[p];
        s = t.start[v];
        if (s == p) return;  // (a first chunk)
        i = s + (p - s + W - 1) / W * W;
    }
    const u64 e = t.start[v + 1];
    const u32 c = static_cast<u32>(e - s);
    if (i >= e || (level > 0 && c <= Wl) || !t.pass(c)) return;
    const u32 o = static_cast<u32>(t.num[v]);
    if (o >= t.cap) return;
    Value acc;
    if (level == 0) {
        const typename Pass::Ctx ctx = pass.begin(o);
        const u32 terms = e - i < OB_CHUNK ? static_cast<u32>(e - i) : OB_CHUNK;
        pass.leaf(t, ctx, static_cast<u32>(t.sorted[i]), acc);
        for (u32 j = 1; j < terms; ++j) {
            Value x;
            pass.leaf(t, ctx, static_cast<u32>(t.sorted[i + j]), x);
            Pass::merge(acc, x);
        }
    } else {
        load_value(lower + tree_slot(i, s, Wl), acc);
        for (u32 j = 1; j < OB_CHUNK; ++j) {
            const u64 q = i + j * Wl;
            if (q >= e) break;
            Value x;
            load_value(lower + tree_slot(q, s, Wl), x);
            Pass::merge(acc, x);
        }
    }
    if (c <= W) pass.finish(o, c, acc);
    else store_value(upper + tree_slot(i, s, W), acc);
}

// One thread per object: the axes of its covariance into entries 3 .. 11 of its 15 doubles.
__global__ __launch_bounds__(OB_BLOCK) void k_obj_axes(const double* __restrict__ cov, const State* __restrict__ st, u32 cap, double* __restrict__ obb)
{
    const u32 o = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (o >= cap || o >= (st->total & 0xFFFFFFFFull)) return;
    double s[6];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        s[a] = cov[static_cast<u64>(o) * 6 + a];
        finite = finite && std::isfinite(s[a]);
    }
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; finite && sweep < HORN_MAX_SWEEPS; ++sweep) {
        const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
        if (!(off > 0.0)) break;
        jacobi_rotate<3, 0, 1>(a, v);
        jacobi_rotate<3, 0, 2>(a, v);
        jacobi_rotate<3, 1, 2>(a, v);
    }
    // column j's place in the descending order of the eigenvalues, the first of equal ones first
    const double l[3] = {a[0][0], a[1][1], a[2][2]};
    int place[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        place[j] = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) place[j] += (l[i] > l[j] || (i < j && l[i] == l[j])) ? 1 : 0;
    }
    double e[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    bool ok = finite;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double x = 0.0, y = 0.0, z = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool take = place[j] == k;
            x = take ? v[0][j] : x;
            y = take ? v[1][j] : y;
            z = take ? v[2][j] : z;
        }
        const double norm = std::sqrt((x * x + y * y) + z * z);
        ok = ok && norm > 0.0;
        x /= norm, y /= norm, z /= norm;
        // the sign: the component of largest magnitude is positive, the lowest index on ties
        double big = x;
        if (std::fabs(y) > std::fabs(big)) big = y;
        if (std::fabs(z) > std::fabs(big)) big = z;
        if (big < 0.0) x = -x, y = -y, z = -z;
        e[k][0] = x, e[k][1] = y, e[k][2] = z;
    }
    if (!ok) {
        e[0][0] = 1.0, e[0][1] = 0.0, e[0][2] = 0.0;
        e[1][0] = 0.0, e[1][1] = 1.0, e[1][2] = 0.0;
    }
    e[2][0] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
    e[2][1] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
    e[2][2] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    double* out = obb + static_cast<u64>(o) * 15 + 3;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * k + j] = e[k][j];
}

struct ObjectsOut {
    u64* count;
    u32 *labels, *counts, *first_row, *offsets, *rows;
    double *centroid, *cov;
    float* aabb;
    double* obb;
    u32* object_of_row;
    u64* skipped;
};

template <class Pass>
void tree_pass(const Layout& L, char* base, const Tree& t, const Pass& pass, hipStream_t s)
{
    for (int level = 0; level < L.levels; ++level) {
        const u64 firsts = level == 0 ? t.n : (t.n + chunk_members(level - 1) - 1) / chunk_members(level - 1);
        const u64 threads = firsts + (t.n + chunk_members(level) - 1) / chunk_members(level);
        const Value* lower = level ? reinterpret_cast<const Value*>(base + L.slots[level - 1]) : nullptr;
        k_obj_tree<Pass><<<blocks_of(threads, OB_BLOCK), OB_BLOCK, 0, s>>>(t, level, firsts, pass, lower, reinterpret_cast<Value*>(base + L.slots[level]));
    }
}

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.
int objects_device(const Layout& L, char* base, const float* d_points, const u32* d_labels, u64 n64, const pcpx_objects_params& a, const ObjectsOut& o,
                   hipStream_t s)
{
    if (n64 == 0) {
        PCPX_HIP(hipMemsetAsync(o.count, 0, sizeof(u64), s));
        if (o.offsets) PCPX_HIP(hipMemsetAsync(o.offsets, 0, sizeof(u32), s));
        if (o.skipped) PCPX_HIP(hipMemsetAsync(o.skipped, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    const u32 n = static_cast<u32>(n64), cap = static_cast<u32>(L.cap), blocks = blocks_of(n, OB_BLOCK);
    State* st = reinterpret_cast<State*>(base + L.state);
    unsigned char* flag = reinterpret_cast<unsigned char*>(base + L.flag);
    u64* word = reinterpret_cast<u64*>(base + L.word[0]);
    u64* sorted = reinterpret_cast<u64*>(base + L.word[1]);
    u32* seg = reinterpret_cast<u32*>(base + L.seg);
    u32* sums32 = reinterpret_cast<u32*>(base + L.sums);
    u64* sums64 = reinterpret_cast<u64*>(base + L.sums);
    u32* start = reinterpret_cast<u32*>(base + L.start);
    double* centroid = o.centroid ? o.centroid : reinterpret_cast<double*>(base + L.centroid);
    double* cov = o.cov ? o.cov : reinterpret_cast<double*>(base + L.cov);
    size_t sort_bytes = L.sort_bytes;
    const Filter pass{a.min_size, a.max_size};
    int r;
    PCPX_HIP(hipMemsetAsync(st, 0, sizeof(State), s));  // (a scan of nothing writes no total)
    k_obj_member<<<blocks, OB_BLOCK, 0, s>>>(d_points, d_labels, n, (a.flags & PCPX_OBJECTS_SKIP) ? 1u : 0u, a.none_label, flag);
    if ((r = exclusive_scan(IsMember{flag}, n, sums32, seg, &st->members, s)) != PCPX_OK) return r;
    k_obj_keys<<<blocks, OB_BLOCK, 0, s>>>(d_labels, flag, seg, n, st, word, o.object_of_row);
    if ((r = sort_keys_u64(base + L.sort, sort_bytes, word, sorted, n, s, 32)) != PCPX_OK) return r;
    if ((r = exclusive_scan(IsHead{sorted, st}, n, sums32, seg, &st->segments, s)) != PCPX_OK) return r;
    k_obj_starts<<<blocks, OB_BLOCK, 0, s>>>(sorted, st, seg, n, start);
    u64* num = word;  // (the unsorted words are done with)
    if ((r = exclusive_scan(ObjectWord{start, st, pass}, n, sums64, num, &st->total, s)) != PCPX_OK) return r;
    k_obj_finish<<<1, 64, 0, s>>>(st, n64, cap, o.count, o.offsets, o.skipped);
    if (o.rows || o.object_of_row) k_obj_rows<<<blocks, OB_BLOCK, 0, s>>>(sorted, seg, start, num, st, n, cap, pass, o.rows, o.object_of_row);
    if (o.labels || o.counts || o.first_row || o.offsets)
        k_obj_heads<<<blocks, OB_BLOCK, 0, s>>>(sorted, start, num, st, n, cap, pass, Heads{o.labels, o.counts, o.first_row, o.offsets});
    if (cap && (o.centroid || o.cov || o.aabb || o.obb)) {
        const Tree t{d_points, sorted, seg, start, num, st, n, cap, pass};
        tree_pass(L, base, t, CentroidPass{centroid, o.aabb}, s);
        if (o.cov || o.obb) tree_pass(L, base, t, CovariancePass{centroid, cov}, s);
        if (o.obb) {
            k_obj_axes<<<blocks_of(cap, OB_BLOCK), OB_BLOCK, 0, s>>>(cov, st, cap, o.obb);
            tree_pass(L, base, t, ExtentPass{centroid, o.obb}, s);
        }
    }
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
int check_size(const char* what, u64 n)
{
    if (n < OB_N_LIMIT) return PCPX_OK;
    set_error("%s: %llu rows: 2^32 - 4096 or more of them", what, static_cast<unsigned long long>(n));
    return PCPX_ERR_INVALID;
}

int check_objects(const char* what, const void* points, const void* labels, u64 n, const pcpx_objects_params* a, const void* stream, const void* count)
{
    const int st = check_size(what, n);
    if (st != PCPX_OK) return st;
    if ((!points || !labels) && n) {
        set_error("%s: a NULL array of points or labels with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    if (!a) {
        set_error("%s: params is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!count) {
        set_error("%s: the count word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (a->flags & ~OB_KNOWN_FLAGS) {
        set_error("%s: unknown flag bits 0x%x", what, a->flags & ~OB_KNOWN_FLAGS);
        return PCPX_ERR_INVALID;
    }
    if (a->reserved != 0u) {
        set_error("%s: reserved = %u is not 0", what, a->reserved);
        return PCPX_ERR_INVALID;
    }
    if (a->min_size == 0u) {
        set_error("%s: min_size is 0", what);
        return PCPX_ERR_INVALID;
    }
    if (a->max_size != 0u && a->max_size < a->min_size) {
        set_error("%s: max_size = %u is below min_size = %u", what, a->max_size, a->min_size);
        return PCPX_ERR_INVALID;
    }
    if (stream && !(a->flags & PCPX_OBJECTS_ON_DEVICE)) {
        set_error("%s: a stream without PCPX_OBJECTS_ON_DEVICE", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_objects_plan(uint64_t n, uint64_t capacity, uint64_t* opt_out_sort_bytes, uint64_t* opt_out_scratch_bytes)
{
    static const char* what = "pcpx_objects_plan";
    return on_host(what, [&]() -> int {
        const int st = check_size(what, n);
        if (st != PCPX_OK) return st;
        const Layout L(n, capacity);
        if (opt_out_sort_bytes) *opt_out_sort_bytes = L.sort_bytes;
        if (opt_out_scratch_bytes) *opt_out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_label_objects(const float* points, const uint32_t* labels, uint64_t n, const pcpx_objects_params* params, uint64_t capacity, int device,
                       void* stream, uint64_t* out_count, uint32_t* opt_out_labels, uint32_t* opt_out_counts, uint32_t* opt_out_first_row,
                       uint32_t* opt_out_offsets, uint32_t* opt_out_rows, double* opt_out_centroid, double* opt_out_cov, float* opt_out_aabb,
                       double* opt_out_obb, uint32_t* opt_out_object_of_row, uint64_t* opt_out_skipped)
{
    static const char* what = "pcpx_label_objects";
    const int st = check_objects(what, points, labels, n, params, stream, out_count);
    if (st != PCPX_OK) return st;
    const Layout L(n, capacity);
    if (params->flags & PCPX_OBJECTS_ON_DEVICE)
        return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
            const ObjectsOut out{out_count,        opt_out_labels, opt_out_counts, opt_out_first_row, opt_out_offsets,       opt_out_rows,
                                 opt_out_centroid, opt_out_cov,    opt_out_aabb,   opt_out_obb,       opt_out_object_of_row, opt_out_skipped};
            return objects_device(L, base, points, labels, n, *params, out, s);
        });
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const u64 cap = L.cap;
        struct Small {
            u64 count, skipped;
        } host{0, 0};
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const u32* d_labels = call.upload(labels, n * sizeof(u32));
        Small* d = call.alloc<Small>(sizeof(Small));
        u32* o_labels = call.alloc_for(opt_out_labels, cap * sizeof(u32));
        u32* o_counts = call.alloc_for(opt_out_counts, cap * sizeof(u32));
        u32* o_first = call.alloc_for(opt_out_first_row, cap * sizeof(u32));
        u32* o_offsets = call.alloc<u32>((cap + 1) * sizeof(u32));  // (always: offsets[S] says how many rows to copy back)
        u32* o_rows = call.alloc_for(opt_out_rows, n * sizeof(u32));
        double* o_centroid = call.alloc_for(opt_out_centroid, cap * 3 * sizeof(double));
        double* o_cov = call.alloc_for(opt_out_cov, cap * 6 * sizeof(double));
        float* o_aabb = call.alloc_for(opt_out_aabb, cap * 6 * sizeof(float));
        double* o_obb = call.alloc_for(opt_out_obb, cap * 15 * sizeof(double));
        u32* o_object = call.alloc_for(opt_out_object_of_row, n * sizeof(u32));
        char* base = call.scratch(L.bytes);
        int r;
        if ((r = call.st) != PCPX_OK) return r;
        PCPX_HIP(hipMemsetAsync(d, 0, sizeof(Small), call.s));
        const ObjectsOut out{&d->count, o_labels, o_counts, o_first, o_offsets, o_rows, o_centroid, o_cov, o_aabb, o_obb, o_object, &d->skipped};
        if ((r = objects_device(L, base, d_points, d_labels, n, *params, out, call.s)) != PCPX_OK ||
            (r = call.download(&host, d, sizeof(Small))) != PCPX_OK || (r = call.wait()) != PCPX_OK)
            return r;
        *out_count = host.count;
        if (capacity < host.count) {
            set_error("%s: %llu objects, room for %llu", what, static_cast<unsigned long long>(host.count), static_cast<unsigned long long>(capacity));
            return PCPX_ERR_CAPACITY;
        }
        const u64 S = host.count;
        u32 members = 0;  // offsets[S]: the rows that are written
        call.download_opt(opt_out_offsets, o_offsets, (S + 1) * sizeof(u32));
        if (opt_out_rows) call.download(&members, o_offsets + S, sizeof(u32));
        if (S) {
            call.download_opt(opt_out_labels, o_labels, S * sizeof(u32));
            call.download_opt(opt_out_counts, o_counts, S * sizeof(u32));
            call.download_opt(opt_out_first_row, o_first, S * sizeof(u32));
            call.download_opt(opt_out_centroid, o_centroid, S * 3 * sizeof(double));
            call.download_opt(opt_out_cov, o_cov, S * 6 * sizeof(double));
            call.download_opt(opt_out_aabb, o_aabb, S * 6 * sizeof(float));
            call.download_opt(opt_out_obb, o_obb, S * 15 * sizeof(double));
        }
        if (n) call.download_opt(opt_out_object_of_row, o_object, n * sizeof(u32));
        if ((r = call.wait()) != PCPX_OK) return r;
        if (opt_out_rows && members) {
            call.download(opt_out_rows, o_rows, static_cast<u64>(members) * sizeof(u32));
            if ((r = call.wait()) != PCPX_OK) return r;
        }
        if (opt_out_skipped) *opt_out_skipped = host.skipped;
        return PCPX_OK;
    });
}

}  // extern "C"
