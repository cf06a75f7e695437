// pcpx_device.h -- device-side helpers shared by the query kernels (kNN, range search, normals): arithmetic of
// the reference (squared distance, box lower bound), scalar (SMEM) record loads, and the wave-uniform walk
// over the implicit 4-ary tree.  Included by .hip translation units only.
#ifndef PCPX_DEVICE_H
#define PCPX_DEVICE_H

#include "pcpx_internal.h"
#include "pcpx_box_bound.h"
#include "pcpx_path_start.h"

#include <cmath>
#include <limits>
#include <type_traits>

#pragma clang fp contract(off)

namespace pcpx {
namespace {

constexpr int WAVES_PER_BLOCK = 1;  // 1: a finished wave frees its LDS at once (no intra-block tail)

__device__ __forceinline__ u32 wave_in_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// XCD-aware block remap: hardware deals blocks round-robin over the 8 XCDs, so give XCD x the
// contiguous range of virtual blocks [x*per, (x+1)*per): curve neighbours then share one L2.
__device__ __forceinline__ u32 virtual_block()
{
    u32 per = gridDim.x >> 3;  // grid is a multiple of 8
    return (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
}

__device__ __forceinline__ float sq3(float dx, float dy, float dz) { return dx * dx + dy * dy + dz * dz; }

// squared distance from q to the box (+ poison): equals d2(q, clamp(q, box)) of
// include/pcp/common/axis_aligned_bounding_box.hpp:138-148 and is a lower bound, in float arithmetic,
// of sq3(p - q) for every p inside the box; NaN for a padding node.
typedef float float_pair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float box_d2(const NodeBox& b, float qx, float qy, float qz)
{
    // (v_med3_f32(q, lo, hi) takes two SGPR operands, which gfx9 VALU encodings do not allow: no cheaper.  Two axes per
    //  packed-float instruction -- v_pk_add_f32 / v_pk_mul_f32 on register pairs, 12 instead of 16 instructions per box -- was
    //  measured in round 4: k_knn the same, k_range 8 % slower; profiles/experiments/README.md)
    float dx = fmaxf(fmaxf(b.lo(0) - qx, qx - b.hi(0)), 0.f);
    float dy = fmaxf(fmaxf(b.lo(1) - qy, qy - b.hi(1)), 0.f);
    float dz = fmaxf(fmaxf(b.lo(2) - qz, qz - b.hi(2)), 0.f);
    return sq3(dx, dy, dz) + b.poison;
}

struct NodeBox4 {
    NodeBox c[W];
};

// The normals of a leaf's eight points by curve position, SoA like the leaf record itself (Leaf, pcpx_internal.h): one 96-byte
// scalar load per leaf, beside its coordinate record (pcpx_segment.hip, pcpx_descriptors.hip).
struct Normals8 {
    float x[LEAF];
    float y[LEAF];
    float z[LEAF];
};
static_assert(sizeof(Normals8) == 12 * LEAF, "normal record must be dense");

// The four child boxes of a node as two 64-byte scalar loads.  (From load_const hipcc fetches only the seven used words of
// each box -- x4 + x2 + x1: twelve SMEM instructions per expansion, and the scalar side of the query kernels is as loaded
// as their vector side.)  The wait is part of the statement: the compiler does not count loads it cannot see.
__device__ __forceinline__ NodeBox4 load_node4(const NodeBox* first_child)
{
    typedef u32 u32x16 __attribute__((ext_vector_type(16)));
    u32x16 a, b;
    // (the address is wave-uniform by construction; where hipcc cannot see that, this pins it to scalar registers)
    const u64 address = reinterpret_cast<uintptr_t>(first_child);
    const u32 address_lo = __builtin_amdgcn_readfirstlane(static_cast<u32>(address));  // (the builtin returns int: no sign extension)
    const u32 address_hi = __builtin_amdgcn_readfirstlane(static_cast<u32>(address >> 32));
    const u64 uniform = (static_cast<u64>(address_hi) << 32) | address_lo;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b)
                 : "s"(uniform));
    NodeBox4 out;
    u32* o = reinterpret_cast<u32*>(&out);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        o[i] = a[i];
        o[16 + i] = b[i];
    }
    return out;
}

// the 32-bit finaliser of MurmurHash3: a bijection, so distinct words give distinct keys (pcpx_subsample.h's
// priorities, pcpx_register.h's sampling)
__host__ __device__ __forceinline__ u32 fmix32(u32 x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool any_lane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }

// Index records (leaves, node boxes) are immutable while a query kernel runs.  Reading them through
// constant-address-space pointers makes every wave-uniform read a scalar (SMEM) load unconditionally;
// through generic pointers hipcc only does that while it can prove no store (or asm with a memory
// clobber, like append_if) may alias them.
template <class T>
__device__ __forceinline__ T load_const(const T* p)
{
    static_assert(sizeof(T) % 4 == 0, "record size");
    typedef const __attribute__((address_space(4))) u32* const_u32_ptr;
    const_u32_ptr c = (const_u32_ptr)(reinterpret_cast<uintptr_t>(p));
    T out;
    u32* o = reinterpret_cast<u32*>(&out);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) o[i] = c[i];
    return out;
}

__device__ __forceinline__ u32 lds_address(const void* p)
{
    return static_cast<u32>(reinterpret_cast<uintptr_t>(p));  // low 32 bits of a generic LDS pointer = LDS offset
}

// ---- wave-uniform walk over the implicit 4-ary tree ------------------------------------------------

// the tight box of a wave's queries (WalkerT::start_path)
struct QueryBox {
    float lo3[3], hi3[3];
    __device__ float lo(int a) const { return lo3[a]; }
    __device__ float hi(int a) const { return hi3[a]; }
};

// All members are wave-uniform (SGPRs).  next() yields, in curve (= sorted) order, every leaf whose box is still
// needed by at least one lane at the time its parent is expanded.  State: bit 4*h + c of `pend` = child c
// (a node of height h; leaves have height 0) of the current ancestor of height h+1 is still to visit.  A
// depth-first walk always continues with the LOWEST set bit of pend, so popping is one find-first-set: no
// per-level loop.  `ploc` is the level-local index of the ancestor of height l+1 (node ids are never
// stored: heap id = (4^d - 1)/3 + local index at tree level d, and a leaf's local index is its number).
// X16: the child boxes come as two 64-byte loads (load_node4) -- fewer scalar instructions, four more SGPRs at once; the
// kernel picks (k_knn for k <= 8, at 8 waves per SIMD, is faster without).
// KEEP: the lanes that needed each of the last expanded node's children are kept (leaf_need) -- k_knn looks at a leaf that few
// lanes need in a form of its own.
template <bool X16, bool KEEP = false>
struct WalkerT {
    u64 pend;
    u32 ploc;
    int l;
    u32 l2;            // 2 * l, carried for pop_scaled() (every member that sets l sets it: a kernel that never reads one of the two does not keep it)
    u32 lshift0;       // 30 - 2 * depth: level_base(depth - h + 1) = 0x55555555 >> (lshift0 + 2 h), for expand_any()
    u64 leaf_need[W];  // KEEP: valid for the children of the most recently expanded node (the leaves popped next, if it was a last-level node)

    // first heap id of tree level d >= 1: (4^d - 1) / 3 = 0b0101...01 (d pairs)
    static __device__ __forceinline__ u32 level_base(int d) { return 0x55555555u >> (32 - 2 * d); }

    // bit c set: child c of the node with local index `loc` at tree level d is needed by some lane
    template <class Need>
    __device__ __forceinline__ u32 child_mask(const TreeView& t, int d, u32 loc, Need&& need)
    {
        return child_mask_at(t, level_base(d + 1) + (loc << LOGW), need);
    }
    // the same for the node whose child 0 has heap id `first_child`
    template <class Need>
    __device__ __forceinline__ u32 child_mask_at(const TreeView& t, u32 first_child, Need&& need)
    {
        const NodeBox4 cb = X16 ? load_node4(t.nodes + first_child) : load_const(reinterpret_cast<const NodeBox4*>(t.nodes + first_child));
        // the mask is built on the scalar unit, two instructions per child: "some lane needs it" goes to SCC and is shifted
        // into the mask with an add-with-carry (children in reverse order, so child 0 ends up in bit 0).  (Left to itself hipcc
        // makes the mask a vector value: v_cndmask, three v_or and a v_readfirstlane per expansion.)
        // (The first child tested SETS the mask, with a select: no register to clear beforehand.)
        u32 m;
#pragma unroll
        for (int c = W - 1; c >= 0; --c) {
            const u64 lanes = __builtin_amdgcn_ballot_w64(need(cb.c[c]));
            if (KEEP) leaf_need[c] = lanes;  // (kept at every expansion, though only a last-level node's are read: keeping them only there
                                             //  measured 2 % SLOWER -- hipcc then moves the masks about at the loop's edges)
            if (c == W - 1) asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(m) : "s"(lanes) : "scc");
            else asm("s_cmp_lg_u64 %1, 0\n\ts_addc_u32 %0, %0, %0" : "+s"(m) : "s"(lanes) : "scc");
        }
        return m;
    }

    // returns true if the root itself is the single leaf (depth 0) and is needed
    template <class Need>
    __device__ __forceinline__ bool start(const TreeView& t, Need&& need, u32& n_expand)
    {
        pend = 0;
        ploc = 0;
        l = 0;
        l2 = 0;
        lshift0 = static_cast<u32>(30 - 2 * t.depth);
        asm("" : "+s"(lshift0));  // (opaque: hipcc otherwise keeps 2 * depth and adds the 30 on every pop)
        if (t.nleaves == 0) return false;
        const NodeBox root = load_const(t.nodes);
        if (!any_lane(need(root))) return false;
        if (t.depth == 0) return true;
        ++n_expand;
        l = t.depth - 1;
        l2 = __builtin_amdgcn_readfirstlane(2u * static_cast<u32>(l));  // (or hipcc carries it round k_knn's walk in a vector register)
        pend = static_cast<u64>(child_mask(t, 0, 0u, need)) << (W * l);
        return false;
    }

    // The start of a SELF group's round (k_knn): one step of the wave in the place of the root test and the depth - 1 expansions of the
    // group's own ancestors, whose outcome is known -- every lane's own point lies inside them (pcpx_path_start.h: the lanes' nodes,
    // the start state).  In two pieces:
    //   path_fetch   each lane loads the box of its node (vector loads); the group's own two last-level nodes -- together the tight box
    //                of its 64 queries, the WAVE BOX -- come as scalar loads.  (A piece of its own so that a caller with registers to
    //                spare can fetch ahead of the round; k_knn has none -- eight VGPRs held across wave_radius_cap put its k <= 16
    //                kernels into scratch -- and fetches where the round starts: profiles/experiments/README.md);
    //   start_path   a lane's node passes if its box-to-box bound to the wave box is within the slackened `cap`
    //                (box_gap_bound_fused, pcpx_box_bound.h).  cap = the round's wave-uniform cap: every searching lane's tau is at most
    //                that from the end of the seed phase on and only shrinks, so the one test covers every lane for the whole round.
    // The test is conservative for the lanes (a passing sibling need not be needed by any: popped, its exact expansion then yields an
    // empty mask) and nothing is dropped that a lane needs.  The walk then runs as from start(), from inside the height-2 ancestor:
    // first that node's other children, then the ancestors' siblings, upwards.  Depth 0: no lane stands for a node, pend = 0.
    struct PathBoxes {
        NodeBox mine;      // per lane
        NodeBox own[2];    // wave-uniform: last-level nodes 2 g and 2 g + 1 (the second may be a padding node)
        u64 lanes;         // the lanes that stand for a node to test
    };
    static __device__ __forceinline__ PathBoxes path_fetch(const TreeView& t, const u32 g, u32 lane)
    {
        asm volatile("" : "+v"(lane));  // (opaque: what depends on the lane alone is otherwise kept in registers from group to group)
        const u32 depth = static_cast<u32>(t.depth);
        const PathLane pl = path_lane(lane, g, depth, 30u - 2u * depth);
        PathBoxes pb;
        pb.lanes = __builtin_amdgcn_ballot_w64(pl.on);
        // (global address space: a load through the generic pointer is a flat one, which the scalar loads below would wait for)
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) f32x4* global_f32x4_ptr;
        // (the node's byte offset as two opaque words: widened as `t.nodes + pl.node`, hipcc keeps the pair {number, 0} in two VGPRs from
        //  group to group of the persistent kernel, and k_knn's k <= 16 kernels have none to spare -- it went to scratch)
        static_assert(sizeof(NodeBox) == 32, "the shifts below");
        u32 off_lo = pl.node << 5, off_hi = pl.node >> 27;
        asm volatile("" : "+v"(off_lo), "+v"(off_hi));
        const global_f32x4_ptr mine = (global_f32x4_ptr)(reinterpret_cast<uintptr_t>(t.nodes) + ((static_cast<u64>(off_hi) << 32) | off_lo));
        const f32x4 a = mine[0], b = mine[1];
        pb.mine.set(a.x, a.y, a.z, a.w, b.x, b.y);
        pb.mine.poison = b.z;
        pb.mine.pad = 0.f;
        const u32 own0 = depth != 0u ? level_base(t.depth - 1) + 2u * g : 0u;  // (depth 0: the root, read and not used)
        // (both numbers opaque scalars, formed where the round starts: the second one's address is otherwise formed in a VGPR pair ahead of
        //  the rounds and kept -- in scratch, in the k <= 16 kernels -- for a later round that hardly any group has)
        u32 own_a = own0, own_b = own0 + (depth != 0u ? 1u : 0u);
        asm volatile("" : "+s"(own_a), "+s"(own_b));
        pb.own[0] = load_const(t.nodes + own_a);
        pb.own[1] = load_const(t.nodes + own_b);
        return pb;
    }
    __device__ __forceinline__ void start_path(const TreeView& t, const u32 g, const PathBoxes& pb, const float cap)
    {
        lshift0 = static_cast<u32>(30 - 2 * t.depth);
        asm("" : "+s"(lshift0));  // (as in start())
        ploc = g >> 1;
        l = 1;
        l2 = 2;
        // the wave box: the union of the group's own last-level nodes (a real node's poison is +0, all bits clear)
        QueryBox w;
        const bool two = __float_as_uint(pb.own[1].poison) == 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            w.lo3[a] = two ? fminf(pb.own[0].lo(a), pb.own[1].lo(a)) : pb.own[0].lo(a);
            w.hi3[a] = two ? fmaxf(pb.own[0].hi(a), pb.own[1].hi(a)) : pb.own[0].hi(a);
        }
        pend = __builtin_amdgcn_ballot_w64(box_gap_bound_fused(pb.mine, w) <= box_bound_tau(cap)) & pb.lanes;
    }

    // The same walk as next(), in pieces, for a caller that keeps "is there another leaf" in its control flow instead of in
    // a value (hipcc turns a wave-uniform bool that lives across blocks into a 64-bit lane mask: s_cselect_b64, s_and_b64
    // with EXEC and a VCC branch where one SCC branch would do; k_knn's scalar side is as loaded as its vector side).
    //   while (!wk.done()) { u32 loc; int h = wk.pop(loc); if (h == 0) { wk.at_leaf(loc); ...leaf loc... } else wk.expand(t, h, loc, need); }
    __device__ __forceinline__ bool done() const { return pend == 0; }
    __device__ __forceinline__ int pop(u32& loc)
    {
        int bit;  // (s_bitset0_b64: from `pend &= ~(1ull << bit)` hipcc makes a shift and an and-not)
        asm("s_ff1_i32_b64 %0, %1\n\ts_bitset0_b64 %1, %0" : "=&s"(bit), "+s"(pend));
        const int h = bit >> LOGW;
        loc = ((ploc >> (LOGW * (h - l))) << LOGW) + (static_cast<u32>(bit) & (W - 1u));  // climb h - l levels, step down
        return h;
    }
    __device__ __forceinline__ void at_leaf(u32 loc)
    {
        ploc = loc >> LOGW;
        l = 0;
        l2 = 0;
    }
    template <class Need>
    __device__ __forceinline__ void expand(const TreeView& t, int h, u32 loc, Need&& need)
    {
        l = h - 1;
        l2 = 2u * static_cast<u32>(l);
        ploc = loc;
        pend |= static_cast<u64>(child_mask(t, t.depth - h, loc, need)) << (W * l);
    }

    // The children of a last-level node (height 1) are leaves: their mask without the trip through the pending bits.  The
    // caller looks at leaves (loc << LOGW) + c for the set bits c and goes on popping (the walker is left as after the last of
    // them: expand() + the pops + at_leaf() of that path cost ~13 scalar instructions per leaf).
    template <class Need>
    __device__ __forceinline__ u32 leaves_of(const TreeView& t, u32 loc, Need&& need)
    {
        l = 0;
        l2 = 0;
        ploc = loc;
        return child_mask(t, t.depth - 1, loc, need);
    }

    // pop() and expand() / leaves_of() for a loop that is short of scalar issue slots (k_knn's walk): ONE expansion for a popped node
    // of any height h >= 1, and the height handled times W, as it stands in the popped bit's number.
    //   while (!wk.done()) { u32 loc; u32 h4 = wk.pop_scaled(loc); u32 leaves = wk.expand_any(t, h4, loc, need); ...leaves (loc << LOGW) + c for the set bits c... }
    // (A loop that calls expand() or leaves_of() by height holds two whole copies of the expansion, and hipcc steers between them
    //  with a wave-uniform bool kept as a lane mask: seven scalar-class instructions of dispatch, three of them branches, on every pop.
    //  With h4 = 4 h the climb's shift is (h4 >> 1) - l2, the level's first heap id 0x55555555 >> (30 - 2 depth + (h4 >> 1)) -- the
    //  first term is the loop's constant -- and the pending bits' shift h4 - 4: four scalar instructions fewer per pop than from h.)
    __device__ __forceinline__ u32 pop_scaled(u32& loc)
    {
        u32 bit;
        asm("s_ff1_i32_b64 %0, %1\n\ts_bitset0_b64 %1, %0" : "=&s"(bit), "+s"(pend));
        const u32 h4 = bit & ~(W - 1u);
        const u32 up = ploc >> ((h4 >> 1) - l2);  // climb h - l levels ...
        asm("s_lshl2_add_u32 %0, %1, %2" : "=s"(loc) : "s"(up), "s"(bit & (W - 1u)) : "scc");  // ... step down (hipcc: shift, and, or)
        static_assert(LOGW == 2, "s_lshl2_add_u32");
        return h4;
    }
    // One child_mask at level depth - h.  The mask of a node above the last level goes to the pending bits, a last-level node's is
    // returned (its needed leaves, as from leaves_of; 0 for a higher node).  ONE scalar branch on the height does that (s_cmp_eq_u32,
    // s_cbranch_scc1): routed by two s_cselect_b32 instead, a last-level node -- more than a third of the pops -- pays for the push it
    // does not need, and the loop was no faster than with the two copies (profiles/experiments/README.md).  The push is an asm
    // statement, or hipcc turns the branch back into selects on a lane mask.
    template <class Need>
    __device__ __forceinline__ u32 expand_any(const TreeView& t, u32 h4, u32 loc, Need&& need)
    {
        const u32 h2 = h4 >> 1;
        const u32 base = 0x55555555u >> (lshift0 + h2);  // level_base(depth - h + 1)
        u32 first_child;
        asm("s_lshl2_add_u32 %0, %1, %2" : "=s"(first_child) : "s"(loc), "s"(base) : "scc");
        const u32 m = child_mask_at(t, first_child, need);
        l = static_cast<int>(h4 >> LOGW) - 1;
        l2 = h2 - 2u;
        ploc = loc;
        u32 direct = m;
        if (h4 != W) {  // above the last level
            u64 pushed;
            asm("s_lshl_b64 %[t], %[m], %[sh]\n\ts_or_b64 %[p], %[p], %[t]" : [p] "+s"(pend), [t] "=&s"(pushed) : [m] "s"(static_cast<u64>(m)), [sh] "s"(h4 - W) : "scc");
            direct = 0;
        }
        return direct;
    }

    template <class Need>
    __device__ __forceinline__ bool next(const TreeView& t, Need&& need, u32& leaf, u32& n_expand)
    {
        while (pend != 0) {
            const int bit = __builtin_ctzll(pend);
            pend &= ~(1ull << bit);
            const int h = bit >> LOGW;
            const u32 loc = ((ploc >> (LOGW * (h - l))) << LOGW) + (static_cast<u32>(bit) & (W - 1u));  // climb h - l levels, step down
            if (h == 0) {
                ploc = loc >> LOGW;
                l = 0;
                l2 = 0;
                leaf = loc;
                return true;
            }
            ++n_expand;
            l = h - 1;
            l2 = 2u * static_cast<u32>(l);
            ploc = loc;
            pend |= static_cast<u64>(child_mask(t, t.depth - h, loc, need)) << (W * l);
        }
        return false;
    }
};
using Walker = WalkerT<true, false>;

// The leaf-direct walk: leaf_fn(leaf, record, who, how_many) is called, in curve order, for every leaf record whose box some
// lane needs -- leaf = its number, record = its address (the callee loads what it reads of it), and with KEEP who = the ballot
// of the lanes that need it and how_many = their number (without: all lanes, GROUP).  "Is there another leaf" is in the
// control flow rather than in a value (WalkerT::pop).  A last-level node looks at its needed leaves itself (leaves_of)
// instead of pushing and popping them: the four children written out, so that a child's record is an immediate offset from
// the node's first leaf and its lanes' ballot a register pair known at compile time.  No tree has depth 1 (depth_of,
// pcpx_build.hip), so no leaf is ever popped.
// BOUNDED: only the leaves below leaf_end.  The walk is depth first in curve order, so the first node that starts at or
// beyond leaf_end ends it.
// (k_range_aabb, pcpx_range.hip, keeps a second form with the children in a scalar loop: 133 scalar registers fewer there.)
template <bool KEEP, bool BOUNDED = false, class Need, class LeafFn>
__device__ __forceinline__ void walk_needed_leaves(const TreeView& t, Need&& need, LeafFn&& leaf_fn, const u32 leaf_end = 0u)
{
    WalkerT<true, KEEP> wk;
    u32 nexp = 0;
    if (wk.start(t, need, nexp) && t.nleaves != 0u && (!BOUNDED || leaf_end != 0u))  // the root is the only leaf
        leaf_fn(0u, t.leaves, ~0ull, static_cast<u32>(GROUP));
    while (!wk.done()) {  // one pop per trip
        u32 loc;
        const int h = wk.pop(loc);
        if (BOUNDED && (static_cast<u64>(loc) << (LOGW * h)) >= leaf_end) break;  // this node and all that are pending lie later
        if (h > 1) {
            wk.expand(t, h, loc, need);
        } else {
            const u32 needed = wk.leaves_of(t, loc, need);
            const Leaf* records = t.leaves + (loc << LOGW);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if ((needed >> c) & 1u) {
                    u32 how_many = GROUP;
                    if (KEEP) asm("s_bcnt1_i32_b64 %0, %1" : "=s"(how_many) : "s"(wk.leaf_need[c]) : "scc");
                    const u32 leaf = (loc << LOGW) + c;
                    if (!BOUNDED || leaf < leaf_end) leaf_fn(leaf, records + c, KEEP ? wk.leaf_need[c] : ~0ull, how_many);
                }
            }
        }
    }
}

// The query of lane p (p below the number of queries): self = the point in leaf slot p, batch = sorted query p of qv.
struct LaneQuery {
    float x, y, z;
    u32 row;  // its output row (self: the point's input index)
};
template <bool SELF>
__device__ __forceinline__ LaneQuery lane_query(const TreeView& t, const QueryView& qv, const u32 p)
{
    if (SELF) {
        const Leaf& lf = t.leaves[p / LEAF];
        return LaneQuery{lf.x[p % LEAF], lf.y[p % LEAF], lf.z[p % LEAF], lf.id[p % LEAF]};
    }
    return LaneQuery{qv.qx[p], qv.qy[p], qv.qz[p], qv.row[p]};
}

inline u32 grid_for_groups(u64 groups)
{
    u64 blocks = (groups + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    blocks = (blocks + 7) / 8 * 8;
    return static_cast<u32>(blocks);
}

inline float sanitize_eps(float eps) { return eps > 0.f ? eps : 0.f; }  // eps <= 0 or NaN: nothing is "equal"

}  // namespace
}  // namespace pcpx

#endif
