// pcpx_api.hip -- the extern "C" boundary declared in include/pcpx.h (and its companions include/pcpx_radius.h and include/pcpx_features.h).
// Host-pointer entry points stage through device buffers and are synchronous; *_dev entry points
// enqueue on the index's stream.  No CPU fallback exists: every compute call needs a HIP device.
#include "pcpx_lease.h"
#include "pcpx_radius.h"
#include "pcpx_features.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace pcpx {
namespace {

// A slice [sorted_first, sorted_first + sorted_count) of the curve order, clamped to the cloud: exactly the positions [lo, hi) are
// answered (the lanes of its first and last query groups outside them idle), and gc groups from group gf hold them
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

// The second half of a batch range search with host outputs: the counts of the nq ranges (device) to offsets (host), the capacity
// check, then the lists that `fill(d_offsets, d_idx)` writes, copied back
template <class Fill>
int lists_to_host(Index* ix, const char* what, u64 nq, const u32* d_cnt, u64* out_offsets, u32* out_idx, u64 idx_capacity, Fill&& fill)
{
    int st;
    std::vector<u32> cnt(nq);
    PCPX_HIP(hipMemcpyAsync(cnt.data(), d_cnt, nq * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    u64 total = 0;
    for (u64 i = 0; i < nq; ++i) {
        out_offsets[i] = total;
        total += cnt[i];
    }
    out_offsets[nq] = total;
    if (total == 0) return PCPX_OK;
    if (!out_idx || idx_capacity < total) {
        set_error("%s: need room for %llu indices", what, static_cast<unsigned long long>(total));
        return PCPX_ERR_CAPACITY;
    }
    DevBuf doff(ix->pool), dout(ix->pool);
    if ((st = doff.alloc((nq + 1) * sizeof(u64))) != PCPX_OK) return st;
    if ((st = dout.alloc(total * sizeof(u32))) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(doff.p, out_offsets, (nq + 1) * sizeof(u64), hipMemcpyHostToDevice, ix->stream));
    if ((st = fill(doff.as<u64>(), dout.as<u32>())) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_idx, dout.p, total * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
}

// d_pos_of (input index -> curve position) and d_nc4 ({normal, count} per curve position) of a whole-cloud handle, made on demand:
// what the gather-form permute of the input-order normals needs.  PCPX_ERR_ALLOC leaves the handle as it was (the caller takes the
// direct form).
int ensure_gather_arrays(Index& ix, size_t bytes_per_position = sizeof(float4))
{
    if (ix.n_in > ix.pos_of_cap || !ix.d_pos_of) {
        PCPX_HIP(hipStreamSynchronize(ix.stream));
        index_block_free(ix.d_pos_of);
        ix.d_pos_of = nullptr;
        ix.pos_of_cap = 0;
        ix.pos_of_valid = false;
        void* p = nullptr;
        if (index_block_alloc(&p, (ix.n_in ? ix.n_in : 1) * sizeof(u32)) != hipSuccess) {
            (void)hipGetLastError();
            return PCPX_ERR_ALLOC;
        }
        ix.d_pos_of = static_cast<u32*>(p);
        ix.pos_of_cap = ix.n_in;
    }
    const u64 need_bytes = (ix.n + GROUP) * bytes_per_position;  // (nc4_cap: bytes of the per-position scratch)
    if (need_bytes > ix.nc4_cap || !ix.d_nc4) {
        PCPX_HIP(hipStreamSynchronize(ix.stream));
        index_block_free(ix.d_nc4);
        ix.d_nc4 = nullptr;
        ix.nc4_cap = 0;
        void* p = nullptr;
        if (index_block_alloc(&p, need_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return PCPX_ERR_ALLOC;
        }
        ix.d_nc4 = static_cast<float4*>(p);
        ix.nc4_cap = need_bytes;
    }
    if (!ix.pos_of_valid) {
        PCPX_HIP(hipMemsetAsync(ix.d_pos_of, 0xFF, ix.n_in * sizeof(u32), ix.stream));
        int st = ix.n ? launch_invert_perm(ix.d_perm, ix.n, ix.d_pos_of, ix.stream) : PCPX_OK;
        if (st != PCPX_OK) return st;
        ix.pos_of_valid = true;
    }
    return PCPX_OK;
}

// Sphere counts of the curve positions of slice `sl` of a whole-cloud handle, BY INPUT INDEX.  Switch "gather_counts" (off): the kernel
// leaves the count of curve position p at [p] of a scratch array (256 contiguous bytes per query group) and k_gather_u32 takes them
// to input order with coalesced writes.  Written straight to input index perm[p] they are 4 bytes per 32-byte sector, read for
// ownership and written back (320 MB at the memory side for 40 MB of counts) -- and still faster than the permute's ten million
// random reads (measured, round 5: 1.92-2.08 ms straight, 2.13 through the permute).
int range_count_self_rows(Index& ix, const Slice& sl, float radius, u32* d_out_count)
{
    QueryView qv = self_view(ix);
    qv.pos_lo = static_cast<u32>(sl.lo);
    qv.pos_hi = static_cast<u32>(sl.hi);
    if (ix.tuning.gather_counts && sl.gc > 0 && ensure_gather_arrays(ix, sizeof(u32)) == PCPX_OK) {
        u32* at_position = reinterpret_cast<u32*>(ix.d_nc4);  // (n + 64 float4: room for n counts)
        qv.by_position = 1;
        int st = launch_range_count(ix, qv, true, sl.gf, sl.gc, radius, nullptr, at_position);
        if (st != PCPX_OK) return st;
        return launch_gather_u32(ix, at_position, ix.d_pos_of, ix.n_in, static_cast<u32>(sl.lo), static_cast<u32>(sl.hi), d_out_count);
    }
    return launch_range_count(ix, qv, true, sl.gf, sl.gc, radius, nullptr, d_out_count);
}

int check_row_stride(const char* what, u32 row_stride, u32 k)
{
    if (row_stride == 0 || (row_stride >= k && k <= 32)) return PCPX_OK;
    set_error("%s: row_stride must be 0 or >= k, and k <= 32", what);
    return PCPX_ERR_INVALID;
}
constexpr auto NO_CHECKS = [] { return PCPX_OK; };

// What the four self-kNN device forms share, after each form's first checks: the slice check, then the form's own checks that
// follow it, the rank-local dispatch and the launch over the slice's query groups.  gather: the input-order normals form, which
// may take the gather-form permute (below).
template <class Checks>
int knn_self_dev(Index* ix, const char* what, u32 k, float eps, u64 sorted_first, u64 sorted_count, KnnOutputs o, Checks&& own_checks,
                 bool gather = false)
{
    int st = check_slice(what, sorted_first);
    if (st == PCPX_OK) st = own_checks();
    if (st != PCPX_OK) return st;
    if (ix->shard.on) {
        if (k > 32 && (!o.idx || !o.cnt)) {
            set_error("%s: a rank-local index answers k > 32 only with the row outputs", what);
            return PCPX_ERR_UNSUPPORTED;
        }
        return shard_knn_self(*ix, sorted_first, sorted_count, k, eps, o);
    }
    const Slice sl = slice_of(*ix, sorted_first, sorted_count);
    const u64 gf = sl.gf, gc = sl.gc;
    o.pos_lo = static_cast<u32>(sl.lo);
    o.pos_hi = static_cast<u32>(sl.hi);
    // Input-order normals (+ counts) by the gather-form permute: the kernel leaves {normal, count} at the query's CURVE position (one
    // contiguous kilobyte per wave) and k_gather_nc4 takes them to input order with coalesced writes.  Written straight to row
    // perm[p] they are 12 + 4 bytes scattered over the whole output: every store instruction touches 64 lines, and every partial
    // 32-byte sector is read for ownership and written back.
    if (gather && ix->tuning.gather && k <= 32 && gc > 0 && ensure_gather_arrays(*ix) == PCPX_OK) {
        float* d_out_normals = o.normals;
        u32* d_opt_out_count = o.cnt;
        o.nc4 = ix->d_nc4;
        o.normals = nullptr;
        o.cnt = nullptr;
        if ((st = launch_knn(*ix, self_view(*ix), true, gf, gc, k, eps, o)) != PCPX_OK) return st;
        return launch_gather_nc4(*ix, ix->d_nc4, ix->d_pos_of, ix->n_in, o.pos_lo, o.pos_hi, d_out_normals, d_opt_out_count);
    }
    if (k > 32 && (!o.idx || !o.cnt)) {  // the multi-pass path materialises rows: keep them in index scratch
        size_t need_idx = (static_cast<size_t>(ix->n_in) * k * sizeof(u32) + 255) / 256 * 256;
        if ((st = ensure_scratch(*ix, need_idx + static_cast<size_t>(ix->n_in) * sizeof(u32))) != PCPX_OK) return st;
        if (!o.idx) o.idx = static_cast<u32*>(ix->d_scratch);
        if (!o.cnt) o.cnt = reinterpret_cast<u32*>(static_cast<char*>(ix->d_scratch) + need_idx);
    }
    return launch_knn(*ix, self_view(*ix), true, gf, gc, k, eps, o);
}

// pcpx_debug_set "poison": every byte that is scratch by contract -- of the handle, of its device's pool and passed leases, of the
// idle index blocks -- gets `byte`; nothing that is state (the tree, the cloud, the work-queue counters, a valid d_pos_of, a recorded
// schedule) and no block that is handed out is touched, and no flag changes.  The handle's stream is drained before and after.
int poison_scratch(Index& ix, int byte)
{
    const hipStream_t s = ix.stream;
    PCPX_HIP(hipStreamSynchronize(s));
    u64 own = 0, shared = 0, cache = 0;
    auto fill = [&](void* p, u64 bytes, u64& sum) -> int {
        if (!p || !bytes) return PCPX_OK;
        PCPX_HIP(hipMemsetAsync(p, byte, bytes, s));
        sum += bytes;
        return PCPX_OK;
    };
    int st;
    if ((st = fill(ix.d_scratch, ix.scratch_bytes, own)) != PCPX_OK || (st = fill(ix.d_multi, ix.multi_bytes, own)) != PCPX_OK ||
        (st = fill(ix.d_nc4, ix.nc4_cap, own)) != PCPX_OK)
        return st;
    if (!ix.pos_of_valid && (st = fill(ix.d_pos_of, ix.pos_of_cap * sizeof(u32), own)) != PCPX_OK) return st;
    if (ix.sched.state == 0 && ((st = fill(ix.sched.d_gtime, ix.sched.cap * sizeof(u32), own)) != PCPX_OK ||
                                (st = fill(ix.sched.d_order, ix.sched.order_entries * sizeof(u32), own)) != PCPX_OK))
        return st;
    if ((st = ix.pool.poison(byte, s, &own)) != PCPX_OK) return st;
    if (ix.device >= 0 && ix.device < LEASE_MAX_DEVICES) {
        DeviceShared& sh = shared_of(ix.device);
        std::lock_guard<std::mutex> lock(sh.mu);
        if ((st = sh.pool.poison(byte, s, &shared)) != PCPX_OK) return st;
        for (auto const& h : g_held[ix.device]) {
            if (hipEventQuery(h.passed) != hipSuccess) {  // (hipErrorNotReady: a queued kernel may still read the block)
                (void)hipGetLastError();
                continue;
            }
            if ((st = fill(h.p, h.bytes, shared)) != PCPX_OK) return st;
        }
        PCPX_HIP(hipStreamSynchronize(s));  // (before the device's lock goes: a call on another stream may take these blocks next)
    }
    if ((st = index_blocks_poison(byte, s, &cache)) != PCPX_OK) return st;  // (waits for s itself)
    ix.poisoned_bytes = own + shared + cache;
    ix.poisoned_shared_bytes = shared;
    ix.poisoned_cache_bytes = cache;
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_abi_version(void) { return PCPX_ABI_VERSION; }
const char* pcpx_last_error(void) { return g_err.c_str(); }

int pcpx_device_count(int* out_count)
{
    if (!out_count) return PCPX_ERR_INVALID;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *out_count = c;
    return PCPX_OK;
}

// A build of the index over `xyz` -- host memory is staged through one of the device's index blocks first -- and then the stream
// drained, also on failure: work of a partial build may still be reading the staging block.  The build's error text survives.
static int build_and_wait(Index& ix, const float* xyz, bool from_host, u64 n, const pcpx_build_params* params)
{
    DevBuf staged(ix.pool, true);
    int st = PCPX_OK;
    if (from_host && n > 0) {
        st = staged.alloc(n * 3 * sizeof(float));
        if (st == PCPX_OK) st = upload_pageable(staged.p, xyz, n * 3 * sizeof(float), ix.stream);
    }
    if (st == PCPX_OK) st = build_index(ix, from_host ? staged.as<float>() : xyz, n, params);
    const std::string why = g_err;
    const int sync = check_hip(hipStreamSynchronize(ix.stream), "build sync", __FILE__, __LINE__);  // (before the staging block goes)
    if (st != PCPX_OK) g_err = why;
    return st != PCPX_OK ? st : sync;
}

static int create_common(const float* xyz, bool on_device, u64 n, const pcpx_build_params* params, int device,
                         void* stream, pcpx_index** out)
{
    if (!out || (n > 0 && !xyz)) {
        set_error("pcpx_index_create: null argument");
        return PCPX_ERR_INVALID;
    }
    *out = nullptr;
    pcpx_build_params full;
    int st = normalise_params(params, on_device, full, params);
    if (st != PCPX_OK) return st;
    return pcpx::on_device(device, "pcpx_index_create", [&]() -> int {
    Index* ix = new (std::nothrow) Index();
    if (!ix) return PCPX_ERR_ALLOC;
    ix->device = device;
    if (on_device) {
        // device-pointer form: work is enqueued on the CALLER's stream; NULL is the legacy default stream, which is
        // ordered against the caller's other default-stream work (a private stream would not be)
        ix->stream = static_cast<hipStream_t>(stream);
    } else {
        // host-pointer form: synchronous calls, so a private stream (no ordering against the caller's streams needed)
        hipError_t e = pooled_stream_get(&ix->stream);
        if (e != hipSuccess) {
            delete ix;
            return check_hip(e, "hipStreamCreate", __FILE__, __LINE__);
        }
        ix->own_stream = true;
    }
    st = build_and_wait(*ix, xyz, !on_device, n, params);
    if (st != PCPX_OK) {
        const std::string why = g_err;  // (free_index's own HIP calls must not replace the reason)
        free_index(ix);
        g_err = why;
        return st;
    }
    *out = reinterpret_cast<pcpx_index*>(ix);
    return PCPX_OK;
    });
}

int pcpx_index_create(const float* xyz, uint64_t n, const pcpx_build_params* params, int device, pcpx_index** out)
{
    return create_common(xyz, false, n, params, device, nullptr, out);
}
int pcpx_index_create_dev(const float* d_xyz, uint64_t n, const pcpx_build_params* params, int device, void* stream,
                          pcpx_index** out)
{
    return create_common(d_xyz, true, n, params, device, stream, out);
}

int pcpx_index_rebuild(pcpx_index* h, const float* xyz, uint64_t n, const pcpx_build_params* params)
{
    return on_index(h, "pcpx_index_rebuild", ANY_INDEX, [&](Index* ix) -> int {
    int st;
    if (n > 0 && !xyz) return PCPX_ERR_INVALID;
    pcpx_build_params full;
    if ((st = normalise_params(params, false, full, params)) != PCPX_OK) return st;
    return build_and_wait(*ix, xyz, true, n, params);
    });
}
int pcpx_index_rebuild_dev(pcpx_index* h, const float* d_xyz, uint64_t n, const pcpx_build_params* params)
{
    return on_index(h, "pcpx_index_rebuild_dev", ANY_INDEX, [&](Index* ix) -> int {
    int st;
    if (n > 0 && !d_xyz) return PCPX_ERR_INVALID;
    pcpx_build_params full;
    if ((st = normalise_params(params, true, full, params)) != PCPX_OK) return st;
    return build_index(*ix, d_xyz, n, params);
    });
}

void pcpx_index_destroy(pcpx_index* h) { free_index(reinterpret_cast<Index*>(h)); }

int pcpx_index_size(pcpx_index* h, uint64_t* out_n)
{
    if (!h || !out_n) return PCPX_ERR_INVALID;
    const Index* ix = reinterpret_cast<Index*>(h);
    *out_n = ix->shard.on ? ix->shard.n_glob : ix->n;  // (a rank-local handle: the whole cloud's inserted points)
    return PCPX_OK;
}
int pcpx_index_shard_info(pcpx_index* h, uint64_t out[8])
{
    const Index* ix = reinterpret_cast<Index*>(h);
    if (!ix || !out || !ix->shard.on) {
        set_error("pcpx_index_shard_info: not a rank-local index");
        return PCPX_ERR_INVALID;
    }
    const Index::Shard& sh = ix->shard;
    out[0] = ix->n;
    out[1] = sh.core_g0;
    out[2] = sh.core_count;
    out[3] = sh.g_first;
    out[4] = sh.g_count;
    out[5] = sh.everything ? 64 : sh.halo_cells;
    out[6] = sh.last_failed;
    out[7] = sh.enlargements;
    return PCPX_OK;
}
int pcpx_index_bbox(pcpx_index* h, float out6[6])
{
    if (!h || !out6) return PCPX_ERR_INVALID;
    std::memcpy(out6, reinterpret_cast<Index*>(h)->bbox, 6 * sizeof(float));
    return PCPX_OK;
}
int pcpx_index_trim(pcpx_index* h)
{
    return on_index(h, "pcpx_index_trim", ANY_INDEX, [&](Index* ix) -> int {
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    ix->pool.trim();
    return PCPX_OK;
    });
}
int pcpx_index_synchronize(pcpx_index* h)
{
    return on_index(h, "pcpx_index_synchronize", ANY_INDEX, [&](Index* ix) -> int {
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_bounding_box_dev(const float* d_xyz, uint64_t n, int device, void* stream, float* d_out6)
{
    if (!d_out6 || (n > 0 && !d_xyz)) return PCPX_ERR_INVALID;
    // d_out6 must have room for the 6 floats; the encoded scratch is a lease: it stays taken until the stream has passed the call
    return on_leased(device, "pcpx_bounding_box_dev", stream, 64 * sizeof(u32), [&](char* base, hipStream_t s) -> int {
    return device_bbox(d_xyz, n, s, reinterpret_cast<u32*>(base), d_out6, false);
    });
}
int pcpx_bounding_box(const float* xyz, uint64_t n, int device, float out6[6])
{
    return on_shared(device, "pcpx_bounding_box", [&](DeviceShared& shared) -> int {
    int st;
    if (!out6 || (n > 0 && !xyz)) return PCPX_ERR_INVALID;
    DevBuf pts(shared.pool), box(shared.pool);
    if ((st = pts.alloc(n * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = box.alloc(64 * sizeof(u32))) != PCPX_OK) return st;
    if (n > 0) PCPX_HIP(hipMemcpy(pts.p, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    float* d_out = box.as<float>() + 32;
    if ((st = device_bbox(pts.as<float>(), n, nullptr, box.as<u32>(), d_out, false)) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpy(out6, d_out, 6 * sizeof(float), hipMemcpyDeviceToHost));
    return PCPX_OK;
    });
}

// ---- kNN -----------------------------------------------------------------------------------------
int pcpx_knn_self_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count,
                      uint32_t* d_out_idx, uint32_t* d_out_count, float* d_out_d2)
{
    return pcpx_knn_self_strided_dev(h, k, eps, sorted_first, sorted_count, 0, d_out_idx, d_out_count, d_out_d2);
}

int pcpx_knn_self_strided_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count, uint32_t row_stride,
                              uint32_t* d_out_idx, uint32_t* d_out_count, float* d_out_d2)
{
    return on_index(h, "pcpx_knn_self_strided_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (k == 0) return PCPX_OK;  // linked_octree_node.hpp:464: k == 0 -> {}
    if (!d_out_idx || !d_out_count) return PCPX_ERR_INVALID;
    KnnOutputs o;
    o.idx = d_out_idx;
    o.cnt = d_out_count;
    o.d2 = d_out_d2;
    o.row_stride = row_stride;
    const char* what = "pcpx_knn_self_strided_dev";
    return knn_self_dev(ix, what, k, eps, sorted_first, sorted_count, o, [&] { return check_row_stride(what, row_stride, k); });
    });
}

int pcpx_knn_self_curve_order_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count, uint32_t* d_out_idx,
                                  uint32_t* d_out_count, float* d_opt_d2, float* d_opt_normals)
{
    return on_index(h, "pcpx_knn_self_curve_order_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (k == 0) return PCPX_OK;
    if (!d_out_idx || !d_out_count) return PCPX_ERR_INVALID;
    KnnOutputs o;
    o.idx = d_out_idx;
    o.cnt = d_out_count;
    o.d2 = d_opt_d2;
    o.normals = d_opt_normals;
    o.by_position = 1;
    return knn_self_dev(ix, "pcpx_knn_self_curve_order_dev", k, eps, sorted_first, sorted_count, o, [&] {
        if (k <= 32 || !o.normals) return PCPX_OK;
        set_error("pcpx_knn_self_curve_order_dev: fused normals need k <= 32");
        return PCPX_ERR_UNSUPPORTED;
    });
    });
}

int pcpx_index_perm_dev(pcpx_index* h, uint32_t* d_out_perm, uint32_t* d_opt_out_position_of)
{
    return on_index(h, "pcpx_index_perm_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (!d_out_perm && !d_opt_out_position_of) return PCPX_ERR_INVALID;
    if (d_opt_out_position_of) PCPX_HIP(hipMemsetAsync(d_opt_out_position_of, 0xFF, ix->n_in * sizeof(u32), ix->stream));
    if (ix->shard.on) return shard_perm(*ix, d_out_perm, d_opt_out_position_of);
    if (ix->n == 0) return PCPX_OK;
    if (d_out_perm) PCPX_HIP(hipMemcpyAsync(d_out_perm, ix->d_perm, ix->n * sizeof(u32), hipMemcpyDeviceToDevice, ix->stream));
    if (d_opt_out_position_of) return launch_invert_perm(ix->d_perm, ix->n, d_opt_out_position_of, ix->stream);
    return PCPX_OK;
    });
}

// Self queries with HOST outputs (pcpx_knn_self, pcpx_normals_knn_self): device staging from the handle's pool (no
// hipMalloc / hipFree per call), one fused launch, one copy per output.  Rows are n x k x 4 bytes: at 10 M points and
// k = 15 the copy to the host (760 MB, ~13.6 ms at this box's 56 GB/s) outweighs the kernel (~5 ms).  The two cannot
// overlap: the kernel walks the curve order and writes row i = input point i, i.e. it scatters over the whole output,
// so no part of an output array is final before the launch ends.  (Tried and measured, profiles/experiments/README.md:
// chunks of the INPUT order through the batch-query form, each chunk's copy overlapping the next chunk's kernels --
// a chunk's queries are ten times sparser than the cloud, a wave's 64 queries then share little of their search
// regions, and the kernels alone took 25.7 ms against 5.3 ms.)
constexpr u64 FEW_QUERIES_MAX = 512;  // up to here pcpx_knn_batch takes the latency path

// any of out_normals / out_idx / out_d2 may be null (out_cnt is required with out_idx)
static int self_queries_to_host(Index* ix, u32 k, float eps, float* out_normals, u32* out_idx, u32* out_cnt, float* out_d2)
{
    int st;
    const u64 rows = ix->n_in;
    if (rows == 0) return PCPX_OK;
    const bool want_rows = out_idx != nullptr;
    DevBuf dn(ix->pool), di(ix->pool), dc(ix->pool), dd(ix->pool);
    if (out_normals && (st = dn.alloc(rows * 3 * sizeof(float))) != PCPX_OK) return st;
    if (want_rows && (st = di.alloc(rows * k * sizeof(u32))) != PCPX_OK) return st;
    if ((want_rows || out_cnt) && (st = dc.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
    if (out_d2 && (st = dd.alloc(rows * k * sizeof(float))) != PCPX_OK) return st;
    if (ix->n != ix->n_in) {  // rows of dropped (out-of-grid) points: count 0, padding
        if (dn.p) PCPX_HIP(hipMemsetAsync(dn.p, 0, rows * 3 * sizeof(float), ix->stream));
        if (di.p) PCPX_HIP(hipMemsetAsync(di.p, 0xFF, rows * k * sizeof(u32), ix->stream));
        if (dc.p) PCPX_HIP(hipMemsetAsync(dc.p, 0, rows * sizeof(u32), ix->stream));
        if (dd.p) PCPX_HIP(hipMemsetAsync(dd.p, 0x7F, rows * k * sizeof(float), ix->stream));
    }
    KnnOutputs o;
    o.idx = di.as<u32>();
    o.cnt = dc.as<u32>();
    o.d2 = dd.as<float>();
    o.normals = dn.as<float>();
    DevBuf srows(ix->pool);
    if (k > 32 && out_normals && !want_rows) {  // the multi-pass path builds normals from materialised rows
        if ((st = srows.alloc(rows * k * sizeof(u32))) != PCPX_OK) return st;
        o.idx = srows.as<u32>();
        if (!dc.p && (st = dc.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
        o.cnt = dc.as<u32>();
    }
    if ((st = launch_knn(*ix, self_view(*ix), true, 0, (ix->n + GROUP - 1) / GROUP, k, eps, o)) != PCPX_OK) return st;
    if (out_normals) PCPX_HIP(hipMemcpyAsync(out_normals, dn.p, rows * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    if (want_rows) PCPX_HIP(hipMemcpyAsync(out_idx, di.p, rows * k * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    if (out_cnt) PCPX_HIP(hipMemcpyAsync(out_cnt, dc.p, rows * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    if (out_d2) PCPX_HIP(hipMemcpyAsync(out_d2, dd.p, rows * k * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
}

int pcpx_knn_self(pcpx_index* h, uint32_t k, float eps, uint32_t* out_idx, uint32_t* out_count, float* out_d2)
{
    return on_index(h, "pcpx_knn_self", WHOLE_CLOUD, [&](Index* ix) -> int {
    if (!out_count || (k > 0 && !out_idx)) return PCPX_ERR_INVALID;
    if (k == 0) {  // linked_octree_node.hpp:464: k == 0 -> {}
        std::memset(out_count, 0, ix->n_in * sizeof(u32));
        return PCPX_OK;
    }
    return self_queries_to_host(ix, k, eps, nullptr, out_idx, out_count, out_d2);
    });
}

int pcpx_knn_batch_dev(pcpx_index* h, const float* d_q_xyz, uint64_t nq, uint32_t k, float eps, uint32_t* d_out_idx,
                       uint32_t* d_out_count, float* d_out_d2)
{
    return on_index(h, "pcpx_knn_batch_dev", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (k == 0 || nq == 0) return PCPX_OK;
    if (!d_q_xyz || !d_out_idx || !d_out_count) return PCPX_ERR_INVALID;
    QueryView qv;
    if ((st = prepare_queries(*ix, d_q_xyz, nq, qv)) != PCPX_OK) return st;
    KnnOutputs o;
    o.idx = d_out_idx;
    o.cnt = d_out_count;
    o.d2 = d_out_d2;
    return launch_knn(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, k, eps, o);
    });
}

int pcpx_knn_batch(pcpx_index* h, const float* q_xyz, uint64_t nq, uint32_t k, float eps, uint32_t* out_idx,
                   uint32_t* out_count, float* out_d2)
{
    return on_index(h, "pcpx_knn_batch", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (nq == 0) return PCPX_OK;
    if (!q_xyz || !out_count || (k > 0 && !out_idx)) return PCPX_ERR_INVALID;
    if (k == 0) {
        std::memset(out_count, 0, nq * sizeof(u32));
        return PCPX_OK;
    }
    if (nq <= FEW_QUERIES_MAX && k <= 32) {
        // latency path (pcpx_few.hip): one wavefront per query, the queries and the rows live in the handle's pinned
        // stage, which the device reads and writes in place -- no allocation, no copy, one launch, one synchronisation
        const size_t o_done = 0, o_q = 64, o_idx = o_q + nq * 3 * sizeof(float), o_cnt = o_idx + nq * k * sizeof(u32),
                     o_d2 = o_cnt + nq * sizeof(u32), o_flag = o_d2 + nq * k * sizeof(float), total = o_flag + nq * sizeof(u32);
        if ((st = ix->pinned.ensure(total)) != PCPX_OK) return st;
        char* stage = static_cast<char*>(ix->pinned.p);
        volatile u32* done = reinterpret_cast<volatile u32*>(stage + o_done);
        if ((st = ensure_queue(*ix)) != PCPX_OK) return st;  // the work-queue counters' allocation also holds the latency path's completion counter (word 15 of queue 7 of the first set)
        u32* done_count = ix->d_queue + 8 * 16 - 1;
        std::memcpy(stage + o_q, q_xyz, nq * 3 * sizeof(float));
        const u32 epoch = next_epoch(ix->few_epoch);
        if ((st = launch_knn_few(*ix, reinterpret_cast<const float*>(stage + o_q), q_xyz, static_cast<u32>(nq), k, eps,
                                 reinterpret_cast<u32*>(stage + o_idx), reinterpret_cast<u32*>(stage + o_cnt),
                                 out_d2 ? reinterpret_cast<float*>(stage + o_d2) : nullptr, reinterpret_cast<u32*>(stage + o_flag),
                                 done_count, const_cast<u32*>(done), epoch)) != PCPX_OK)
            return st;
        if ((st = wait_epoch(done, epoch, ix->stream)) != PCPX_OK) return st;  // (the kernel's last block stores the epoch)
        bool complete = true;
        const u32* flags = reinterpret_cast<const u32*>(stage + o_flag);
        for (u64 q = 0; q < nq; ++q) complete = complete && flags[q] == 0u;
        if (complete) {
            std::memcpy(out_idx, stage + o_idx, nq * k * sizeof(u32));
            std::memcpy(out_count, stage + o_cnt, nq * sizeof(u32));
            if (out_d2) std::memcpy(out_d2, stage + o_d2, nq * k * sizeof(float));
            return PCPX_OK;
        }
        // a frontier or candidate list overflowed (a query far outside a large cloud, hundreds of exact ties): general path
    }
    DevBuf dq(ix->pool), di(ix->pool), dc(ix->pool), dd(ix->pool);
    if ((st = dq.alloc(nq * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = di.alloc(nq * k * sizeof(u32))) != PCPX_OK) return st;
    if ((st = dc.alloc(nq * sizeof(u32))) != PCPX_OK) return st;
    if (out_d2 && (st = dd.alloc(nq * k * sizeof(float))) != PCPX_OK) return st;
    if ((st = upload_pageable(dq.p, q_xyz, nq * 3 * sizeof(float), ix->stream)) != PCPX_OK) return st;
    st = pcpx_knn_batch_dev(h, dq.as<float>(), nq, k, eps, di.as<u32>(), dc.as<u32>(), out_d2 ? dd.as<float>() : nullptr);
    if (st != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_idx, di.p, nq * k * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipMemcpyAsync(out_count, dc.p, nq * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    if (out_d2) PCPX_HIP(hipMemcpyAsync(out_d2, dd.p, nq * k * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

// ---- radius search -------------------------------------------------------------------------------
int pcpx_range_count_self_dev(pcpx_index* h, float radius, uint64_t sorted_first, uint64_t sorted_count,
                              uint32_t* d_out_count)
{
    return on_index(h, "pcpx_range_count_self_dev", ANY_INDEX, [&](Index* ix) -> int {
    int st;
    if (!d_out_count) return PCPX_ERR_INVALID;
    if ((st = check_slice("pcpx_range_count_self_dev", sorted_first)) != PCPX_OK) return st;
    if (ix->shard.on) return shard_range_count_self(*ix, radius, sorted_first, sorted_count, d_out_count);
    return range_count_self_rows(*ix, slice_of(*ix, sorted_first, sorted_count), radius, d_out_count);
    });
}

// The same with the count of sorted position p at d_out_count[p]: a query group's 64 counts are one 256-byte store (the
// input-order form scatters 4-byte stores over the whole array: eight times the bytes at the memory side).
int pcpx_range_count_self_curve_order_dev(pcpx_index* h, float radius, uint64_t sorted_first, uint64_t sorted_count,
                                          uint32_t* d_out_count)
{
    return on_index(h, "pcpx_range_count_self_curve_order_dev", ANY_INDEX, [&](Index* ix) -> int {
    int st;
    if (!d_out_count) return PCPX_ERR_INVALID;
    if ((st = check_slice("pcpx_range_count_self_curve_order_dev", sorted_first)) != PCPX_OK) return st;
    if (ix->shard.on) return shard_range_count_self(*ix, radius, sorted_first, sorted_count, d_out_count, true);
    const Slice sl = slice_of(*ix, sorted_first, sorted_count);
    QueryView qv = self_view(*ix);
    qv.by_position = 1;
    qv.pos_lo = static_cast<u32>(sl.lo);
    qv.pos_hi = static_cast<u32>(sl.hi);
    return launch_range_count(*ix, qv, true, sl.gf, sl.gc, radius, nullptr, d_out_count);
    });
}

int pcpx_range_lists_self_dev(pcpx_index* h, float radius, uint64_t* d_out_offsets, uint32_t* d_out_idx, uint64_t idx_capacity,
                              uint64_t* out_total)
{
    return on_index(h, "pcpx_range_lists_self_dev", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!d_out_offsets || !out_total) return PCPX_ERR_INVALID;
    *out_total = 0;
    const u64 rows = ix->n_in;
    if (rows == 0) {
        PCPX_HIP(hipMemsetAsync(d_out_offsets, 0, sizeof(u64), ix->stream));
        PCPX_HIP(hipStreamSynchronize(ix->stream));
        return PCPX_OK;
    }
    // scratch of the handle: the counts by input row and the scan's tile sums
    const size_t cnt_bytes = (rows * sizeof(u32) + 255) / 256 * 256, sums = (rows / 1024 + 2) * sizeof(u64);
    if ((st = ensure_scratch(*ix, cnt_bytes + sums)) != PCPX_OK) return st;
    u32* d_cnt = static_cast<u32*>(ix->d_scratch);
    u64* d_sums = reinterpret_cast<u64*>(static_cast<char*>(ix->d_scratch) + cnt_bytes);
    if (ix->n != ix->n_in) PCPX_HIP(hipMemsetAsync(d_cnt, 0, rows * sizeof(u32), ix->stream));  // (points outside the grid: empty lists)
    const Slice all = slice_of(*ix, 0, UINT64_MAX);
    if ((st = range_count_self_rows(*ix, all, radius, d_cnt)) != PCPX_OK) return st;
    if ((st = launch_range_offsets(*ix, d_cnt, rows, d_sums, d_out_offsets)) != PCPX_OK) return st;
    u64 total = 0;
    PCPX_HIP(hipMemcpyAsync(&total, d_out_offsets + rows, sizeof(u64), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    *out_total = total;
    if (total == 0) return PCPX_OK;
    if (!d_out_idx || idx_capacity < total) {
        set_error("pcpx_range_lists_self_dev: need room for %llu indices", static_cast<unsigned long long>(total));
        return PCPX_ERR_CAPACITY;
    }
    return launch_range_fill_self(*ix, 0, all.gc, radius, d_out_offsets, d_out_idx);
    });
}

int pcpx_range_count_self(pcpx_index* h, float radius, uint32_t* out_count)
{
    return on_index(h, "pcpx_range_count_self", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_count) return PCPX_ERR_INVALID;
    u64 rows = ix->n_in;
    DevBuf dc(ix->pool);
    if ((st = dc.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
    PCPX_HIP(hipMemsetAsync(dc.p, 0, rows * sizeof(u32), ix->stream));
    if ((st = pcpx_range_count_self_dev(h, radius, 0, UINT64_MAX, dc.as<u32>())) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_count, dc.p, rows * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_range_count_batch(pcpx_index* h, const float* q_xyz, uint64_t nq, float radius, uint32_t* out_count)
{
    return on_index(h, "pcpx_range_count_batch", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (nq == 0) return PCPX_OK;
    if (!q_xyz || !out_count) return PCPX_ERR_INVALID;
    DevBuf dq(ix->pool), dc(ix->pool);
    if ((st = dq.alloc(nq * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = dc.alloc(nq * sizeof(u32))) != PCPX_OK) return st;
    if ((st = upload_pageable(dq.p, q_xyz, nq * 3 * sizeof(float), ix->stream)) != PCPX_OK) return st;
    QueryView qv;
    if ((st = prepare_queries(*ix, dq.as<float>(), nq, qv)) != PCPX_OK) return st;
    if ((st = launch_range_count(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, radius, nullptr, dc.as<u32>())) != PCPX_OK)
        return st;
    PCPX_HIP(hipMemcpyAsync(out_count, dc.p, nq * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

// One sphere / one box per call: the latency form (pcpx_range.hip: k_range_one) through the handle's pinned stage.  Returns
// PCPX_OK / PCPX_ERR_CAPACITY like the batch form, or +1 when the range holds more than the stage does (caller: batch form).
constexpr u32 RANGE_ONE_CAP = 4096;
static int range_one_to_host(Index* ix, bool aabb, const float* range6, uint64_t* out_offsets, uint32_t* out_idx, uint64_t idx_capacity)
{
    int st;
    const size_t o_done = 0, o_cnt = 128, o_idx = 192, total = o_idx + RANGE_ONE_CAP * sizeof(u32);
    if ((st = ix->pinned.ensure(total)) != PCPX_OK) return st;
    char* stage = static_cast<char*>(ix->pinned.p);
    volatile u32* done = reinterpret_cast<volatile u32*>(stage + o_done);
    const u32 epoch = next_epoch(ix->few_epoch);  // (shared with the k-NN latency path: same word)
    if ((st = launch_range_one(*ix, aabb, range6, RANGE_ONE_CAP, reinterpret_cast<u32*>(stage + o_idx),
                               reinterpret_cast<u32*>(stage + o_cnt), const_cast<u32*>(done), epoch)) != PCPX_OK)
        return st;
    if ((st = wait_epoch(done, epoch, ix->stream)) != PCPX_OK) return st;
    const u32 cnt = *reinterpret_cast<const volatile u32*>(stage + o_cnt);
    if (cnt > RANGE_ONE_CAP) return 1;
    out_offsets[0] = 0;
    out_offsets[1] = cnt;
    if (cnt == 0) return PCPX_OK;
    if (!out_idx || idx_capacity < cnt) {
        set_error("pcpx range search: need room for %u indices", cnt);
        return PCPX_ERR_CAPACITY;
    }
    std::memcpy(out_idx, stage + o_idx, cnt * sizeof(u32));
    return PCPX_OK;
}

int pcpx_range_sphere_batch(pcpx_index* h, const float* q_xyz, const float* radii, float radius, uint64_t nq,
                            uint64_t* out_offsets, uint32_t* out_idx, uint64_t idx_capacity)
{
    return on_index(h, "pcpx_range_sphere_batch", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_offsets || (nq > 0 && !q_xyz)) return PCPX_ERR_INVALID;
    if (nq == 0) {
        out_offsets[0] = 0;
        return PCPX_OK;
    }
    if (nq == 1) {  // the per-call shape of the reference's API: one launch through the pinned stage
        const float sphere[4] = {q_xyz[0], q_xyz[1], q_xyz[2], radii ? radii[0] : radius};
        st = range_one_to_host(ix, false, sphere, out_offsets, out_idx, idx_capacity);
        if (st != 1) return st;
    }
    DevBuf dq(ix->pool), dr(ix->pool), dc(ix->pool);
    if ((st = dq.alloc(nq * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = dc.alloc(nq * sizeof(u32))) != PCPX_OK) return st;
    if ((st = upload_pageable(dq.p, q_xyz, nq * 3 * sizeof(float), ix->stream)) != PCPX_OK) return st;
    if (radii) {
        if ((st = dr.alloc(nq * sizeof(float))) != PCPX_OK) return st;
        PCPX_HIP(hipMemcpyAsync(dr.p, radii, nq * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    }
    QueryView qv;
    if ((st = prepare_queries(*ix, dq.as<float>(), nq, qv)) != PCPX_OK) return st;
    if ((st = launch_range_count(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, radius, dr.as<float>(), dc.as<u32>())) != PCPX_OK)
        return st;
    return lists_to_host(ix, "pcpx_range_sphere_batch", nq, dc.as<u32>(), out_offsets, out_idx, idx_capacity,
                         [&](const u64* d_offsets, u32* d_idx) { return launch_range_fill(*ix, qv, radius, dr.as<float>(), d_offsets, d_idx); });
    });
}

int pcpx_range_aabb_batch(pcpx_index* h, const float* boxes6, uint64_t nb, uint64_t* out_offsets, uint32_t* out_idx,
                          uint64_t idx_capacity)
{
    return on_index(h, "pcpx_range_aabb_batch", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_offsets || (nb > 0 && !boxes6)) return PCPX_ERR_INVALID;
    if (nb == 0) {
        out_offsets[0] = 0;
        return PCPX_OK;
    }
    if (nb == 1) {
        st = range_one_to_host(ix, true, boxes6, out_offsets, out_idx, idx_capacity);
        if (st != 1) return st;
    }
    DevBuf db(ix->pool), dc(ix->pool);
    if ((st = db.alloc(nb * 6 * sizeof(float))) != PCPX_OK) return st;
    if ((st = dc.alloc(nb * sizeof(u32))) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(db.p, boxes6, nb * 6 * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    if ((st = launch_aabb_count(*ix, db.as<float>(), nb, dc.as<u32>())) != PCPX_OK) return st;
    return lists_to_host(ix, "pcpx_range_aabb_batch", nb, dc.as<u32>(), out_offsets, out_idx, idx_capacity,
                         [&](const u64* d_offsets, u32* d_idx) { return launch_aabb_fill(*ix, db.as<float>(), nb, d_offsets, d_idx); });
    });
}

// ---- normals -------------------------------------------------------------------------------------
int pcpx_normals_knn_self_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count,
                              float* d_out_normals, uint32_t* d_opt_out_idx, uint32_t* d_opt_out_count)
{
    return pcpx_normals_knn_self_strided_dev(h, k, eps, sorted_first, sorted_count, 0, d_out_normals, d_opt_out_idx, d_opt_out_count);
}

int pcpx_normals_knn_self_strided_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count, uint32_t row_stride,
                                      float* d_out_normals, uint32_t* d_opt_out_idx, uint32_t* d_opt_out_count)
{
    return on_index(h, "pcpx_normals_knn_self_strided_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (!d_out_normals || k == 0) return PCPX_ERR_INVALID;
    // fused kernel: kNN rows stay in registers, only what the caller asked for is written
    KnnOutputs o;
    o.idx = d_opt_out_idx;
    o.cnt = d_opt_out_count;
    o.normals = d_out_normals;
    o.row_stride = row_stride;
    const char* what = "pcpx_normals_knn_self_strided_dev";
    return knn_self_dev(ix, what, k, eps, sorted_first, sorted_count, o, [&] { return check_row_stride(what, row_stride, k); }, true);
    });
}

// estimate_tangent_planes / average_distances_to_neighbors over the index's own points
int pcpx_neighbourhoods_self_dev(pcpx_index* h, uint32_t k, float eps, uint64_t sorted_first, uint64_t sorted_count,
                                 float* d_opt_normals, float* d_opt_centroids, float* d_opt_mean_dist)
{
    return on_index(h, "pcpx_neighbourhoods_self_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (k == 0 || (!d_opt_normals && !d_opt_centroids && !d_opt_mean_dist)) return PCPX_ERR_INVALID;
    KnnOutputs o;
    o.normals = d_opt_normals;
    o.centroids = d_opt_centroids;
    o.meandist = d_opt_mean_dist;
    return knn_self_dev(ix, "pcpx_neighbourhoods_self_dev", k, eps, sorted_first, sorted_count, o, NO_CHECKS);
    });
}

int pcpx_tangent_planes_knn_self(pcpx_index* h, uint32_t k, float eps, float* out_centroids, float* out_normals)
{
    return on_index(h, "pcpx_tangent_planes_knn_self", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_centroids || !out_normals || k == 0) return PCPX_ERR_INVALID;
    u64 rows = ix->n_in;
    DevBuf dc(ix->pool), dn(ix->pool);
    if ((st = dc.alloc(rows * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = dn.alloc(rows * 3 * sizeof(float))) != PCPX_OK) return st;
    PCPX_HIP(hipMemsetAsync(dc.p, 0, rows * 3 * sizeof(float), ix->stream));
    PCPX_HIP(hipMemsetAsync(dn.p, 0, rows * 3 * sizeof(float), ix->stream));
    if ((st = pcpx_neighbourhoods_self_dev(h, k, eps, 0, UINT64_MAX, dn.as<float>(), dc.as<float>(), nullptr)) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_centroids, dc.p, rows * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipMemcpyAsync(out_normals, dn.p, rows * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_mean_knn_distance_self(pcpx_index* h, uint32_t k, float eps, float* out_mean_dist)
{
    return on_index(h, "pcpx_mean_knn_distance_self", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_mean_dist || k == 0) return PCPX_ERR_INVALID;
    u64 rows = ix->n_in;
    DevBuf dm(ix->pool);
    if ((st = dm.alloc(rows * sizeof(float))) != PCPX_OK) return st;
    PCPX_HIP(hipMemsetAsync(dm.p, 0, rows * sizeof(float), ix->stream));
    if ((st = pcpx_neighbourhoods_self_dev(h, k, eps, 0, UINT64_MAX, nullptr, nullptr, dm.as<float>())) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_mean_dist, dm.p, rows * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_normals_knn_self(pcpx_index* h, uint32_t k, float eps, float* out_normals, uint32_t* opt_out_idx,
                          uint32_t* opt_out_count)
{
    return on_index(h, "pcpx_normals_knn_self", WHOLE_CLOUD, [&](Index* ix) -> int {
    if (!out_normals || k == 0) return PCPX_ERR_INVALID;
    return self_queries_to_host(ix, k, eps, out_normals, opt_out_idx, opt_out_count, nullptr);
    });
}

// Rows in curve order: the kernel writes the rows of a slice of the sorted order into one contiguous piece of every output
// array, so a finished slice travels to the host while the later slices are still being computed (the input-order form
// scatters rows over the whole output: its copy cannot start before the last kernel has ended).
int pcpx_normals_knn_self_curve_order(pcpx_index* h, uint32_t k, float eps, float* opt_out_normals, uint32_t* out_idx, uint32_t* out_count,
                                      uint32_t* opt_out_perm, uint32_t* opt_out_position_of)
{
    return on_index(h, "pcpx_normals_knn_self_curve_order", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (k == 0 || !out_idx || !out_count) return PCPX_ERR_INVALID;
    const u64 rows = ix->n;  // inserted points only: a point outside the voxel grid has no position on the curve
    if (opt_out_position_of && ix->n != ix->n_in) std::memset(opt_out_position_of, 0xFF, ix->n_in * sizeof(u32));
    if (rows == 0) return PCPX_OK;
    if (!ix->copy_stream) PCPX_HIP(pooled_stream_get(&ix->copy_stream));
    DevBuf dn(ix->pool), di(ix->pool), dc(ix->pool), dinv(ix->pool);
    if (opt_out_normals && (st = dn.alloc(rows * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = di.alloc(rows * k * sizeof(u32))) != PCPX_OK || (st = dc.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
    if (opt_out_position_of && (st = dinv.alloc(ix->n_in * sizeof(u32))) != PCPX_OK) return st;
    KnnOutputs o;
    o.idx = di.as<u32>();
    o.cnt = dc.as<u32>();
    o.normals = dn.as<float>();
    o.by_position = 1;
    const u64 groups = (rows + GROUP - 1) / GROUP;
    constexpr int MAX_SLICES = 8;
    const int slices = static_cast<int>(groups < 8 * 1024 ? 1 : MAX_SLICES);  // (a slice should still fill the chip a few times over)
    hipEvent_t done[MAX_SLICES] = {};
    struct EventGuard {
        hipEvent_t* e;
        ~EventGuard()
        {
            for (int i = 0; i < MAX_SLICES; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{done};
    // Whatever way this function is left -- an error half way through included -- both streams are drained first: queued
    // kernels and copies write the caller's arrays and read buffers that go back to the pool (declared last: destroyed first,
    // before the events and the buffers above).
    struct Drain {
        Index* ix;
        ~Drain()
        {
            (void)hipStreamSynchronize(ix->copy_stream);
            (void)hipStreamSynchronize(ix->stream);
        }
    } drain{ix};
    // all the kernels first (enqueueing does not block) ...
    u64 g_first[MAX_SLICES + 1];
    for (int s = 0; s <= slices; ++s) g_first[s] = groups * static_cast<u64>(s) / static_cast<u64>(slices);
    for (int s = 0; s < slices; ++s) {
        if ((st = launch_knn(*ix, self_view(*ix), true, g_first[s], g_first[s + 1] - g_first[s], k, eps, o)) != PCPX_OK) return st;
        PCPX_HIP(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
        PCPX_HIP(hipEventRecord(done[s], ix->stream));
    }
    if (opt_out_position_of) {
        if (ix->n != ix->n_in) PCPX_HIP(hipMemsetAsync(dinv.p, 0xFF, ix->n_in * sizeof(u32), ix->stream));
        if ((st = launch_invert_perm(ix->d_perm, rows, dinv.as<u32>(), ix->stream)) != PCPX_OK) return st;
    }
    // ... then the copies, slice by slice, on the second stream, each behind its slice's kernel
    if (opt_out_perm) PCPX_HIP(hipMemcpyAsync(opt_out_perm, ix->d_perm, rows * sizeof(u32), hipMemcpyDeviceToHost, ix->copy_stream));
    for (int s = 0; s < slices; ++s) {
        const u64 r0 = g_first[s] * GROUP, r1 = std::min<u64>(rows, g_first[s + 1] * GROUP);
        PCPX_HIP(hipStreamWaitEvent(ix->copy_stream, done[s], 0));
        PCPX_HIP(hipMemcpyAsync(out_idx + r0 * k, di.as<u32>() + r0 * k, (r1 - r0) * k * sizeof(u32), hipMemcpyDeviceToHost, ix->copy_stream));
        PCPX_HIP(hipMemcpyAsync(out_count + r0, dc.as<u32>() + r0, (r1 - r0) * sizeof(u32), hipMemcpyDeviceToHost, ix->copy_stream));
        if (opt_out_normals)
            PCPX_HIP(hipMemcpyAsync(opt_out_normals + 3 * r0, dn.as<float>() + 3 * r0, (r1 - r0) * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->copy_stream));
    }
    PCPX_HIP(hipStreamSynchronize(ix->copy_stream));
    if (opt_out_position_of) PCPX_HIP(hipMemcpyAsync(opt_out_position_of, dinv.p, ix->n_in * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_normals_from_knn(pcpx_index* h, const uint32_t* nbr_idx, const uint32_t* count, uint64_t nq, uint32_t k,
                          float* out_normals, float* opt_out_evals)
{
    return on_index(h, "pcpx_normals_from_knn", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (nq == 0) return PCPX_OK;
    if (!nbr_idx || !count || !out_normals || k == 0) return PCPX_ERR_INVALID;
    for (u64 q = 0; q < nq; ++q) {
        if (count[q] > k) {
            set_error("pcpx_normals_from_knn: count[%llu] > k", static_cast<unsigned long long>(q));
            return PCPX_ERR_INVALID;
        }
        for (u32 j = 0; j < count[q]; ++j)
            if (nbr_idx[q * k + j] >= ix->n_in) {
                set_error("pcpx_normals_from_knn: neighbour index out of range in row %llu", static_cast<unsigned long long>(q));
                return PCPX_ERR_INVALID;
            }
    }
    DevBuf di(ix->pool), dc(ix->pool), dn(ix->pool), de(ix->pool);
    if ((st = di.alloc(nq * k * sizeof(u32))) != PCPX_OK) return st;
    if ((st = dc.alloc(nq * sizeof(u32))) != PCPX_OK) return st;
    if ((st = dn.alloc(nq * 3 * sizeof(float))) != PCPX_OK) return st;
    if (opt_out_evals && (st = de.alloc(nq * 3 * sizeof(float))) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(di.p, nbr_idx, nq * k * sizeof(u32), hipMemcpyHostToDevice, ix->stream));
    PCPX_HIP(hipMemcpyAsync(dc.p, count, nq * sizeof(u32), hipMemcpyHostToDevice, ix->stream));
    st = launch_normals(*ix, di.as<u32>(), dc.as<u32>(), nullptr, 0, nq, k, dn.as<float>(),
                        opt_out_evals ? de.as<float>() : nullptr);
    if (st != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_normals, dn.p, nq * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    if (opt_out_evals) PCPX_HIP(hipMemcpyAsync(opt_out_evals, de.p, nq * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_estimate_normal(const float* xyz, uint64_t m, int device, float out_normal[3])
{
    return on_shared(device, "pcpx_estimate_normal", [&](DeviceShared& shared) -> int {
    int st;
    if (!out_normal || (m > 0 && !xyz)) return PCPX_ERR_INVALID;
    if (m >= 1 && m <= NORMAL_ARG_POINTS) {
        // the reference's per-point shape (k neighbours, then their normal): the points travel in the kernel arguments, the
        // normal and a completion word come back through the device's pinned stage, which the host polls
        if ((st = shared.pinned.ensure(64 * sizeof(float))) != PCPX_OK) return st;
        float* stage = static_cast<float*>(shared.pinned.p);
        volatile u32* done = reinterpret_cast<volatile u32*>(stage + 8);
        const u32 epoch = next_epoch(shared.normal_epoch);
        if (*done == epoch) *done = 0u;  // (a fresh stage may hold anything)
        if ((st = launch_normal_args(xyz, static_cast<u32>(m), stage, const_cast<u32*>(done), epoch, nullptr)) != PCPX_OK) return st;
        if ((st = wait_epoch(done, epoch, nullptr)) != PCPX_OK) return st;
        std::memcpy(out_normal, stage, 3 * sizeof(float));
        return PCPX_OK;
    }
    if (m <= 4096) {
        // one neighbourhood: no allocation and no copy -- the points go into the device's pinned stage, the kernel reads
        // them and writes the normal there (host memory mapped into the device's address space)
        if ((st = shared.pinned.ensure((m * 3 + 4) * sizeof(float))) != PCPX_OK) return st;
        float* stage = static_cast<float*>(shared.pinned.p);
        if (m > 0) std::memcpy(stage + 4, xyz, m * 3 * sizeof(float));
        if ((st = launch_normal_single(stage + 4, m, stage, nullptr)) != PCPX_OK) return st;
        PCPX_HIP(hipStreamSynchronize(nullptr));
        std::memcpy(out_normal, stage, 3 * sizeof(float));
        return PCPX_OK;
    }
    DevBuf dp(shared.pool), dn(shared.pool);
    if ((st = dp.alloc(m * 3 * sizeof(float))) != PCPX_OK) return st;
    if ((st = dn.alloc(3 * sizeof(float))) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpy(dp.p, xyz, m * 3 * sizeof(float), hipMemcpyHostToDevice));
    if ((st = launch_normal_single(dp.as<float>(), m, dn.as<float>(), nullptr)) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpy(out_normal, dn.p, 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PCPX_OK;
    });
}

int pcpx_estimate_normals_batch(const float* xyz, const uint64_t* offsets, uint64_t nrows, int device, float* out_normals)
{
    return on_shared(device, "pcpx_estimate_normals_batch", [&](DeviceShared& shared) -> int {
    int st;
    if (nrows == 0) return PCPX_OK;
    if (!offsets || !out_normals) return PCPX_ERR_INVALID;
    for (u64 r = 0; r < nrows; ++r)
        if (offsets[r + 1] < offsets[r]) {
            set_error("pcpx_estimate_normals_batch: offsets must not decrease (row %llu)", static_cast<unsigned long long>(r));
            return PCPX_ERR_INVALID;
        }
    const u64 total = offsets[nrows] - offsets[0];
    if (total > 0 && !xyz) return PCPX_ERR_INVALID;
    DevBuf dp(shared.pool), doff(shared.pool), dn(shared.pool);
    if ((st = dp.alloc(total * 3 * sizeof(float))) != PCPX_OK || (st = doff.alloc((nrows + 1) * sizeof(u64))) != PCPX_OK ||
        (st = dn.alloc(nrows * 3 * sizeof(float))) != PCPX_OK)
        return st;
    if (total > 0) PCPX_HIP(hipMemcpyAsync(dp.p, xyz + 3 * offsets[0], total * 3 * sizeof(float), hipMemcpyHostToDevice, nullptr));
    PCPX_HIP(hipMemcpyAsync(doff.p, offsets, (nrows + 1) * sizeof(u64), hipMemcpyHostToDevice, nullptr));
    if ((st = launch_normals_csr(dp.as<float>(), doff.as<u64>(), nrows, dn.as<float>(), nullptr)) != PCPX_OK) return st;
    PCPX_HIP(hipMemcpyAsync(out_normals, dn.p, nrows * 3 * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    PCPX_HIP(hipStreamSynchronize(nullptr));
    return PCPX_OK;
    });
}

int pcpx_debug_eps_test_mode(pcpx_index* h, int mode)
{
    return on_index(h, "pcpx_debug_eps_test_mode", ANY_INDEX, [&](Index* ix) -> int {
    if (mode < 0 || mode > 2) {
        set_error("pcpx_debug_eps_test_mode: mode is 0 (automatic), 1 (in the compaction) or 2 (per candidate)");
        return PCPX_ERR_INVALID;
    }
    ix->eps_test_mode = mode;
    return PCPX_OK;
    });
}

int pcpx_debug_set(pcpx_index* h, const char* name, int64_t value)
{
    return on_index(h, "pcpx_debug_set", ANY_INDEX, [&](Index* ix) -> int {
    if (!name) return PCPX_ERR_INVALID;
    const std::string key(name);
    if (key == "long_groups_first") {
        ix->tuning.lpt = value != 0;
        ix->sched.state = 0;
    } else if (key == "gather_outputs") {
        ix->tuning.gather = value != 0;
    } else if (key == "gather_counts") {
        ix->tuning.gather_counts = value != 0;
    } else if (key == "icp_resort") {
        ix->tuning.icp_resort = value != 0;
    } else if (key == "icp_previous_start") {
        ix->tuning.icp_previous_start = value < 0 ? -1 : value != 0;
    } else if (key == "fps_bucket_height") {
        if (value < 0 || value > 3) {
            set_error("pcpx_debug_set: fps_bucket_height is 0 (automatic), 1, 2 or 3");
            return PCPX_ERR_INVALID;
        }
        ix->tuning.fps_bucket_height = static_cast<int>(value);
    } else if (key == "fps_prune") {
        ix->tuning.fps_prune = value != 0;
    } else if (key == "fps_one_block") {
        ix->tuning.fps_one_block = value < 0 ? -1 : value != 0;
    } else if (key == "poison") {
        if (value < 0 || value > 255) {
            set_error("pcpx_debug_set: poison takes a byte, 0 ... 255");
            return PCPX_ERR_INVALID;
        }
        return poison_scratch(*ix, static_cast<int>(value));
    } else {
        set_error("pcpx_debug_set: no setting called '%s'", name);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
    });
}

int pcpx_debug_get(pcpx_index* h, const char* name, int64_t* out_value)
{
    return on_index(h, "pcpx_debug_get", ANY_INDEX, [&](Index* ix) -> int {
    if (!name || !out_value) return PCPX_ERR_INVALID;
    const std::string key(name);
    if (key == "build_redos") {
        *out_value = ix->build_redos;
    } else if (key == "full_buckets") {
        int64_t c = 0;
        for (u32 w = 0; w < 8; ++w) c += __builtin_popcount(ix->full_buckets[w]);
        *out_value = c;
    } else if (key == "schedule_state") {
        *out_value = ix->sched.state;
    } else if (key == "poisoned_bytes") {
        *out_value = static_cast<int64_t>(ix->poisoned_bytes);
    } else if (key == "poisoned_shared_bytes") {
        *out_value = static_cast<int64_t>(ix->poisoned_shared_bytes);
    } else if (key == "poisoned_cache_bytes") {
        *out_value = static_cast<int64_t>(ix->poisoned_cache_bytes);
    } else if (key == "scratch_bytes") {
        *out_value = static_cast<int64_t>(ix->scratch_bytes);
    } else if (key == "knn_row_form") {
        *out_value = ix->knn_row_form;
    } else {
        set_error("pcpx_debug_get: no figure called '%s'", name);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
    });
}

int pcpx_debug_group_times(pcpx_index* h, uint32_t* out_ticks, uint64_t capacity, uint64_t* out_groups)
{
    return on_index(h, "pcpx_debug_group_times", ANY_INDEX, [&](Index* ix) -> int {
    if (!out_groups) return PCPX_ERR_INVALID;
    *out_groups = ix->sched.state ? ix->sched.gc : 0;
    if (*out_groups == 0) return PCPX_OK;
    if (!out_ticks || capacity < *out_groups) return PCPX_ERR_CAPACITY;
    PCPX_HIP(hipMemcpyAsync(out_ticks, ix->sched.d_gtime, *out_groups * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_knn_group_costs_dev(pcpx_index* h, uint32_t k, float eps, uint32_t group_stride, uint32_t* d_out_events, uint64_t capacity,
                             uint64_t* out_samples)
{
    return on_index(h, "pcpx_knn_group_costs_dev", ANY_INDEX, [&](Index* ix) -> int {
    if (!out_samples || group_stride == 0) return PCPX_ERR_INVALID;
    if (ix->shard.on) return shard_unsupported(*ix, "pcpx_knn_group_costs_dev");  // (after the argument checks)
    const u64 groups = (ix->n + GROUP - 1) / GROUP;
    const u64 nsamples = groups / group_stride;
    *out_samples = nsamples;
    if (!d_out_events || capacity < nsamples) return nsamples == 0 ? PCPX_OK : PCPX_ERR_CAPACITY;
    u32 ns = 0;
    return launch_knn_cost_sample(*ix, k, eps, group_stride, d_out_events, &ns);
    });
}

int pcpx_debug_knn_stats(pcpx_index* h, uint32_t k, float eps, uint64_t* out_stats, uint64_t capacity)
{
    return on_index(h, "pcpx_debug_knn_stats", WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!out_stats || capacity < 16 || k == 0 || k > 16) return PCPX_ERR_INVALID;
    DevBuf ds(ix->pool);
    const size_t cap = 16 + 5 * 65536;  // 16 counters + 5-word records of up to 65536 persistent waves
    if ((st = ds.alloc(cap * sizeof(u64))) != PCPX_OK) return st;
    PCPX_HIP(hipMemsetAsync(ds.p, 0, cap * sizeof(u64), ix->stream));
    // capacity bit 63 set: "floor" mode -- start every lane from its true k-th distance (taken from a normal run first)
    const bool floor_mode = (capacity >> 63) != 0;
    capacity &= ~(1ull << 63);
    DevBuf known(ix->pool);
    if (floor_mode) {
        if ((st = known.alloc(static_cast<size_t>(ix->n_in) * k * sizeof(float))) != PCPX_OK) return st;
        KnnOutputs o;
        o.d2 = known.as<float>();
        if ((st = launch_knn(*ix, self_view(*ix), true, 0, (ix->n + GROUP - 1) / GROUP, k, eps, o)) != PCPX_OK) return st;
    }
    if ((st = launch_knn_stats(*ix, k, eps, ds.as<unsigned long long>(), floor_mode ? known.as<float>() : nullptr)) != PCPX_OK) return st;
    const size_t ncopy = capacity < cap ? capacity : cap;
    PCPX_HIP(hipMemcpyAsync(out_stats, ds.p, ncopy * sizeof(u64), hipMemcpyDeviceToHost, ix->stream));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    return PCPX_OK;
    });
}

int pcpx_debug_sort_keys(const uint64_t* keys, uint64_t n, int first_bit, int device, uint64_t* out_keys)
{
    return on_shared(device, "pcpx_debug_sort_keys", [&](DeviceShared& shared) -> int {
    int st;
    if (n > 0 && (!keys || !out_keys)) return PCPX_ERR_INVALID;
    size_t tb = 0;
    if ((st = sort_keys_u64(nullptr, tb, nullptr, nullptr, n, nullptr, first_bit)) != PCPX_OK) return st;
    DevBuf ki(shared.pool), ko(shared.pool), tmp(shared.pool);
    if ((st = ki.alloc(n * 8)) != PCPX_OK || (st = ko.alloc(n * 8)) != PCPX_OK || (st = tmp.alloc(tb)) != PCPX_OK) return st;
    if (n > 0) PCPX_HIP(hipMemcpy(ki.p, keys, n * 8, hipMemcpyHostToDevice));
    if ((st = sort_keys_u64(tmp.p, tb, ki.as<u64>(), ko.as<u64>(), n, nullptr, first_bit)) != PCPX_OK) return st;
    PCPX_HIP(hipDeviceSynchronize());
    if (n > 0) {
        u32 failed = 0;
        PCPX_HIP(hipMemcpy(&failed, sort_failure_flag(tmp.p), sizeof(u32), hipMemcpyDeviceToHost));
        if (failed) {
            set_error("pcpx: internal error, the radix sort's look-back gave up");
            return PCPX_ERR_DEVICE;
        }
        PCPX_HIP(hipMemcpy(out_keys, ko.p, n * 8, hipMemcpyDeviceToHost));
    }
    return PCPX_OK;
    });
}

// (for tests: include/pcpx.h)
int pcpx_debug_tree(pcpx_index* h, uint64_t* out_shape, void* out_leaves, uint64_t leaf_capacity, void* out_nodes, uint64_t node_capacity,
                    uint32_t* out_first_pass)
{
    return on_index(h, "pcpx_debug_tree", ANY_INDEX, [&](Index* ix) -> int {
    if (!out_shape) return PCPX_ERR_INVALID;
    static_assert(PCPX_DEBUG_TREE_SHAPE_WORDS == 4 + MAXDEPTH + 1, "one word per level");
    u32 nleaves = 0, written[MAXDEPTH + 1];
    int depth = 0;
    build_tree_shape(static_cast<u32>(ix->n), &nleaves, &depth, written);
    const u64 level0 = ((1ull << (2 * depth)) - 1ull) / 3ull;  // heap id of the first node of level `depth`
    const u64 nnodes = nleaves ? level0 + written[depth] : 0;
    out_shape[0] = ix->n;
    out_shape[1] = nleaves;
    out_shape[2] = static_cast<u64>(depth);
    out_shape[3] = nnodes;
    for (int d = 0; d <= MAXDEPTH; ++d) out_shape[4 + d] = written[d];
    if (nleaves != ix->nleaves || depth != ix->depth || nnodes > ix->nodes_cap) {
        set_error("pcpx_debug_tree: internal error, the handle's tree is not the shape of its point count");
        return PCPX_ERR_DEVICE;
    }
    if (!out_leaves || !out_nodes || !out_first_pass || leaf_capacity < nleaves || node_capacity < nnodes) return PCPX_ERR_CAPACITY;
    const hipStream_t s = ix->stream;
    const bool finish_sort = ix->finish_words && ix->n_in > 0;  // (a build of no points runs no sort: the pointers are an earlier build's)
    if (finish_sort) PCPX_HIP(hipMemcpyAsync(out_first_pass, ix->finish_first_pass, 256 * sizeof(u32), hipMemcpyDeviceToHost, s));
    else std::memset(out_first_pass, 0, 256 * sizeof(u32));
    if (nleaves) {
        PCPX_HIP(hipMemcpyAsync(out_leaves, ix->d_leaves, static_cast<size_t>(nleaves) * sizeof(Leaf), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipMemcpyAsync(out_nodes, ix->d_nodes, static_cast<size_t>(nnodes) * sizeof(NodeBox), hipMemcpyDeviceToHost, s));
    }
    PCPX_HIP(hipStreamSynchronize(s));
    return PCPX_OK;
    });
}

int pcpx_profile_begin(pcpx_index* h)
{
    return on_index(h, "pcpx_profile_begin", ANY_INDEX, [&](Index* ix) -> int {
    for (auto& iv : ix->intervals) {
        (void)hipEventDestroy(iv.a);
        (void)hipEventDestroy(iv.b);
    }
    ix->intervals.clear();
    ix->profiling = true;
    return PCPX_OK;
    });
}

int pcpx_profile_end(pcpx_index* h, pcpx_profile* out)
{
    return on_index(h, "pcpx_profile_end", ANY_INDEX, [&](Index* ix) -> int {
    if (!out) return PCPX_ERR_INVALID;
    ix->profiling = false;
    std::memset(out, 0, sizeof(*out));
    PCPX_HIP(hipStreamSynchronize(ix->stream));
    for (auto& iv : ix->intervals) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, iv.a, iv.b) == hipSuccess && iv.family >= 0 && iv.family < PCPX_K_FAMILIES) {
            out->launches[iv.family] += 1;
            out->total_ms[iv.family] += ms;
        }
        (void)hipEventDestroy(iv.a);
        (void)hipEventDestroy(iv.b);
    }
    ix->intervals.clear();
    return PCPX_OK;
    });
}

int pcpx_device_malloc(uint64_t bytes, int device, void** out_ptr)
{
    if (!out_ptr) return PCPX_ERR_INVALID;
    *out_ptr = nullptr;
    return on_device(device, "pcpx_device_malloc", [&]() -> int {
    hipError_t e = hipMalloc(out_ptr, bytes ? bytes : 16);
    if (e != hipSuccess) {
        *out_ptr = nullptr;
        (void)hipGetLastError();
        set_error("hipMalloc(%llu bytes) failed: %s", static_cast<unsigned long long>(bytes), hipGetErrorString(e));
        return PCPX_ERR_ALLOC;
    }
    return PCPX_OK;
    });
}
int pcpx_device_trim(int device)
{
    return on_device(device, "pcpx_device_trim", [&]() -> int {
    index_blocks_trim();
    return PCPX_OK;
    });
}

void pcpx_device_free(void* d_ptr, int device)
{
    if (!d_ptr) return;
    DeviceScope dscope;
    if (dscope.select(device) != PCPX_OK) return;
    (void)hipFree(d_ptr);
}
int pcpx_device_upload(void* d_dst, const void* src, uint64_t bytes, int device, void* stream)
{
    if (bytes == 0) return PCPX_OK;
    if (!d_dst || !src) return PCPX_ERR_INVALID;
    return on_device(device, "pcpx_device_upload", [&]() -> int {
    int st;
    if ((st = upload_pageable(d_dst, src, bytes, static_cast<hipStream_t>(stream))) != PCPX_OK) return st;
    PCPX_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PCPX_OK;
    });
}
int pcpx_device_download(void* dst, const void* d_src, uint64_t bytes, int device, void* stream)
{
    if (bytes == 0) return PCPX_OK;
    if (!dst || !d_src) return PCPX_ERR_INVALID;
    return on_device(device, "pcpx_device_download", [&]() -> int {
    PCPX_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    PCPX_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PCPX_OK;
    });
}

// ---- fixed-radius neighbourhoods (include/pcpx_radius.h): the moments form of the sphere walk ------------------------------------
static int no_outputs(const char* what)
{
    set_error("%s: every output is NULL", what);
    return PCPX_ERR_INVALID;
}

// The moments form for the curve positions of slice `sl`, by input row, on the handle's stream: what both forms below run
static int range_neighbourhoods_self(Index& ix, float radius, const Slice& sl, float* d_opt_normals, float* d_opt_centroids,
                                     float* d_opt_mean_dist, u32* d_opt_count)
{
    int st;
    if (sl.lo == 0 && sl.hi == ix.n && ix.n != ix.n_in) {  // the whole curve order: the rows of the points outside the grid too
        if ((st = ensure_gather_arrays(ix, sizeof(u32))) != PCPX_OK) return st;
        if ((st = launch_range_moments_empty_rows(ix, ix.d_pos_of, ix.n_in, d_opt_normals, d_opt_centroids, d_opt_mean_dist, d_opt_count)) !=
            PCPX_OK)
            return st;
    }
    QueryView qv = self_view(ix);
    qv.pos_lo = static_cast<u32>(sl.lo);
    qv.pos_hi = static_cast<u32>(sl.hi);
    return launch_range_moments(ix, qv, true, sl.gf, sl.gc, radius, nullptr, d_opt_normals, d_opt_centroids, d_opt_mean_dist, d_opt_count);
}

int pcpx_range_neighbourhoods_self_dev(pcpx_index* h, float radius, uint64_t sorted_first, uint64_t sorted_count,
                                       float* d_opt_normals, float* d_opt_centroids, float* d_opt_mean_dist, uint32_t* d_opt_count)
{
    static const char* what = "pcpx_range_neighbourhoods_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    if (!d_opt_normals && !d_opt_centroids && !d_opt_mean_dist && !d_opt_count) return no_outputs(what);
    if ((st = check_radius(what, radius)) != PCPX_OK) return st;
    if ((st = check_slice(what, sorted_first)) != PCPX_OK) return st;
    return range_neighbourhoods_self(*ix, radius, slice_of(*ix, sorted_first, sorted_count), d_opt_normals, d_opt_centroids, d_opt_mean_dist,
                                     d_opt_count);
    });
}

// Host outputs of the moments form: one device block per asked output, `run` fills them, then the copies back and the wait
extern "C++" template <class Run>
static int moments_staged(Staged& stage, u64 rows, float* normals, float* centroids, float* mean_dist, u32* count, Run&& run)
{
    int st;
    float* dn = stage.alloc_for(normals, rows * 3 * sizeof(float));
    float* dc = stage.alloc_for(centroids, rows * 3 * sizeof(float));
    float* dm = stage.alloc_for(mean_dist, rows * sizeof(float));
    u32* dk = stage.alloc_for(count, rows * sizeof(u32));
    if ((st = stage.st) != PCPX_OK || (st = run(dn, dc, dm, dk)) != PCPX_OK) return st;
    stage.download_opt(normals, dn, rows * 3 * sizeof(float));
    stage.download_opt(centroids, dc, rows * 3 * sizeof(float));
    stage.download_opt(mean_dist, dm, rows * sizeof(float));
    stage.download_opt(count, dk, rows * sizeof(u32));
    return stage.wait();
}

int pcpx_range_neighbourhoods_self(pcpx_index* h, float radius, float* opt_normals, float* opt_centroids, float* opt_mean_dist,
                                   uint32_t* opt_count)
{
    static const char* what = "pcpx_range_neighbourhoods_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
    int st;
    if (!opt_normals && !opt_centroids && !opt_mean_dist && !opt_count) return no_outputs(what);
    if ((st = check_radius(what, radius)) != PCPX_OK) return st;
    if (ix->n_in == 0) return PCPX_OK;
    return moments_staged(stage, ix->n_in, opt_normals, opt_centroids, opt_mean_dist, opt_count, [&](float* dn, float* dc, float* dm, u32* dk) {
        return range_neighbourhoods_self(*ix, radius, slice_of(*ix, 0, UINT64_MAX), dn, dc, dm, dk);
    });
    });
}

// The batch forms' spheres: checked (every radius >= 0) ...
static int check_spheres(const char* what, const float* q_xyz, const float* radii, float radius, u64 nq)
{
    if (nq > 0 && !q_xyz) return PCPX_ERR_INVALID;
    if (radii) {
        for (u64 i = 0; i < nq; ++i)
            if (!(radii[i] >= 0.f)) {
                set_error("%s: radius %llu must be >= 0 (got %g)", what, static_cast<unsigned long long>(i), static_cast<double>(radii[i]));
                return PCPX_ERR_INVALID;
            }
    } else {
        return check_radius(what, radius);
    }
    return PCPX_OK;
}
// ... then staged on the device (*d_radii: null without a radii array) and prepared as queries; nq > 0
static int stage_spheres(Index& ix, Staged& stage, const float* q_xyz, const float* radii, u64 nq, const float** d_radii, QueryView& qv)
{
    const float* dq = stage.upload(q_xyz, nq * 3 * sizeof(float));
    *d_radii = stage.upload(radii, nq * sizeof(float));
    return stage.st != PCPX_OK ? stage.st : prepare_queries(ix, dq, nq, qv);
}

int pcpx_range_neighbourhoods_batch(pcpx_index* h, const float* q_xyz, const float* radii, float radius, uint64_t nq,
                                    float* opt_normals, float* opt_centroids, float* opt_mean_dist, uint32_t* opt_count)
{
    static const char* what = "pcpx_range_neighbourhoods_batch";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
    int st;
    if (!opt_normals && !opt_centroids && !opt_mean_dist && !opt_count) return no_outputs(what);
    if ((st = check_spheres(what, q_xyz, radii, radius, nq)) != PCPX_OK) return st;
    if (nq == 0) return PCPX_OK;
    const float* dr;
    QueryView qv;
    if ((st = stage_spheres(*ix, stage, q_xyz, radii, nq, &dr, qv)) != PCPX_OK) return st;
    return moments_staged(stage, nq, opt_normals, opt_centroids, opt_mean_dist, opt_count, [&](float* dn, float* dc, float* dm, u32* dk) {
        return launch_range_moments(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, radius, dr, dn, dc, dm, dk);
    });
    });
}

// ---- local shape features (include/pcpx_features.h): the features form of the sphere walk -------------------------------------------
struct FeaturesPtrs {
    float* evals;
    float* curvature;
    float* normals;
    float* axes;
    uint32_t* count;
    bool none() const { return !evals && !curvature && !normals && !axes && !count; }
};
static int check_features_outputs(const char* what, const FeaturesPtrs& out) { return out.none() ? no_outputs(what) : PCPX_OK; }

// The features form for the curve positions of slice `sl`, by input row, on the handle's stream: what both forms below run
static int shape_features_self(Index& ix, float radius, const Slice& sl, const FeaturesPtrs& d)
{
    int st;
    if (sl.lo == 0 && sl.hi == ix.n && ix.n != ix.n_in) {  // the whole curve order: the rows of the points outside the grid too
        if ((st = ensure_gather_arrays(ix, sizeof(u32))) != PCPX_OK) return st;
        if ((st = launch_range_features_empty_rows(ix, ix.d_pos_of, ix.n_in, d.evals, d.curvature, d.normals, d.axes, d.count)) != PCPX_OK)
            return st;
    }
    QueryView qv = self_view(ix);
    qv.pos_lo = static_cast<u32>(sl.lo);
    qv.pos_hi = static_cast<u32>(sl.hi);
    return launch_range_features(ix, qv, true, sl.gf, sl.gc, radius, nullptr, d.evals, d.curvature, d.normals, d.axes, d.count);
}

int pcpx_shape_features_self_dev(pcpx_index* h, float radius, uint64_t sorted_first, uint64_t sorted_count, float* d_opt_evals,
                                 float* d_opt_curvature, float* d_opt_normals, float* d_opt_axes, uint32_t* d_opt_count)
{
    static const char* what = "pcpx_shape_features_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
    int st;
    const FeaturesPtrs d{d_opt_evals, d_opt_curvature, d_opt_normals, d_opt_axes, d_opt_count};
    if ((st = check_features_outputs(what, d)) != PCPX_OK) return st;
    if ((st = check_radius(what, radius)) != PCPX_OK) return st;
    if ((st = check_slice(what, sorted_first)) != PCPX_OK) return st;
    return shape_features_self(*ix, radius, slice_of(*ix, sorted_first, sorted_count), d);
    });
}

// Host outputs of the features form: one device block per asked output, `run` fills them, then the copies back and the wait
extern "C++" template <class Run>
static int features_staged(Staged& stage, u64 rows, const FeaturesPtrs& out, Run&& run)
{
    int st;
    const FeaturesPtrs d{stage.alloc_for(out.evals, rows * 3 * sizeof(float)), stage.alloc_for(out.curvature, rows * sizeof(float)),
                         stage.alloc_for(out.normals, rows * 3 * sizeof(float)), stage.alloc_for(out.axes, rows * 3 * sizeof(float)),
                         stage.alloc_for(out.count, rows * sizeof(u32))};
    if ((st = stage.st) != PCPX_OK || (st = run(d)) != PCPX_OK) return st;
    stage.download_opt(out.evals, d.evals, rows * 3 * sizeof(float));
    stage.download_opt(out.curvature, d.curvature, rows * sizeof(float));
    stage.download_opt(out.normals, d.normals, rows * 3 * sizeof(float));
    stage.download_opt(out.axes, d.axes, rows * 3 * sizeof(float));
    stage.download_opt(out.count, d.count, rows * sizeof(u32));
    return stage.wait();
}

int pcpx_shape_features_self(pcpx_index* h, float radius, float* opt_evals, float* opt_curvature, float* opt_normals, float* opt_axes,
                             uint32_t* opt_count)
{
    static const char* what = "pcpx_shape_features_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
    int st;
    const FeaturesPtrs out{opt_evals, opt_curvature, opt_normals, opt_axes, opt_count};
    if ((st = check_features_outputs(what, out)) != PCPX_OK) return st;
    if ((st = check_radius(what, radius)) != PCPX_OK) return st;
    if (ix->n_in == 0) return PCPX_OK;
    return features_staged(stage, ix->n_in, out, [&](const FeaturesPtrs& d) {
        return shape_features_self(*ix, radius, slice_of(*ix, 0, UINT64_MAX), d);
    });
    });
}

int pcpx_shape_features_batch(pcpx_index* h, const float* q_xyz, const float* radii, float radius, uint64_t nq, float* opt_evals,
                              float* opt_curvature, float* opt_normals, float* opt_axes, uint32_t* opt_count)
{
    static const char* what = "pcpx_shape_features_batch";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
    int st;
    const FeaturesPtrs out{opt_evals, opt_curvature, opt_normals, opt_axes, opt_count};
    if ((st = check_features_outputs(what, out)) != PCPX_OK) return st;
    if ((st = check_spheres(what, q_xyz, radii, radius, nq)) != PCPX_OK) return st;
    if (nq == 0) return PCPX_OK;
    const float* dr;
    QueryView qv;
    if ((st = stage_spheres(*ix, stage, q_xyz, radii, nq, &dr, qv)) != PCPX_OK) return st;
    return features_staged(stage, nq, out, [&](const FeaturesPtrs& d) {
        return launch_range_features(*ix, qv, false, 0, (nq + GROUP - 1) / GROUP, radius, dr, d.evals, d.curvature, d.normals, d.axes, d.count);
    });
    });
}

}  // extern "C"
