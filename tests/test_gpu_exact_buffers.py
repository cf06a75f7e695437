"""Every device-pointer entry point on buffers that are exactly as large and exactly as aligned as the C headers promise
(include/pcpx.h, conventions: a device pointer needs its element type's alignment and no more; a call writes only inside the
documented extents of its outputs).

Every other GPU test hands the library tensors straight from torch's allocator: 256-byte aligned, slack behind them, another tensor in
front.  Here they come from the arena of tests/exact_buffers.py -- guard | payload | guard, the payload 4 (or 8, or 1) bytes off a
16-byte boundary -- and

  a. every row of tests/exact_buffers_cases.py leaves the guards alone, leaves the caller's elements alone, and writes bit for bit
     what the same call writes into plain torch.full buffers -- the form the rest of the suite pins to its models;
  b. the bounding-box reduction reads its cloud as 16-byte vectors after peeling up to three points (k_bbox): pcpx_bounding_box_dev
     and the two device builds at every 4-byte offset and every small size give the exact box, and the builds the exact rows;
  c. two rank-local handles that BORROW a cloud at such an address (they read it in place for as long as they live) answer as the
     whole-cloud index does.

No cloud is larger than 5 000 points; the kNN rows rest on no exact tie (tests/test_exact_buffers_cpu.py)."""
import numpy as np
import pytest

import exact_buffers as EB
import exact_buffers_cases as XC
import handle_history_cases as HH
import nonfinite_cases as N

pytestmark = pytest.mark.gpu
F = np.float32
DEVICE = "cuda:0"


def _torch():
    return pytest.importorskip("torch")


_handles = {}


def _handle(pkg, cloud):
    if cloud not in _handles:
        _handles[cloud] = HH.build(pkg, cloud)
    return _handles[cloud]


# ---- a. extents and alignment, every row --------------------------------------------------------------------------------------------------
CASES = [(row, cloud) for row in XC.ROWS for cloud in XC.clouds_of(row)]


@pytest.mark.parametrize("row,cloud", CASES, ids=["%s-%s" % c for c in CASES])
def test_a_row_on_exact_buffers_writes_the_same_bits_and_nothing_else(pkg, row, cloud):
    t = _torch()
    ix = None if XC.ROWS[row].family == "free" else _handle(pkg, cloud)
    plain, plain_owned = XC.run(pkg, ix, cloud, row)
    t.cuda.synchronize()
    arena = EB.Arena(DEVICE)
    got, owned = XC.run(pkg, ix, cloud, row, arena)
    t.cuda.synchronize()
    arena.check((row, cloud))
    assert sorted(got) == sorted(plain) and sorted(owned) == sorted(plain_owned)
    for key, a in got.items():
        p = plain[key]
        assert a.dtype == p.dtype and a.shape == p.shape, (row, cloud, key, a.dtype, p.dtype, a.shape, p.shape)
        mask = owned.get(key)
        if mask is None:
            mask = np.zeros(len(a), bool)
        assert np.array_equal(mask, plain_owned.get(key, mask)), (row, cloud, key)  # (the counts behind the masks agree)
        # the caller's elements: still the arena's fill here, still the plain buffers' fill there
        EB.Arena.untouched(a, mask, (row, cloud, key))
        lead = mask if len(mask) == len(a) else mask.reshape(a.shape)
        assert (p[lead] == p.dtype.type(HH.FILL)).all(), (row, cloud, key, "plain buffers")
        # every other element: the same bits
        ba, bp = HH.bits(a)[~lead], HH.bits(p)[~lead]
        bad = np.nonzero((ba != bp).reshape(-1))[0]
        assert len(bad) == 0, (row, cloud, key, len(bad), bad[:8].tolist())


FORM_CASES = [(row, cloud) for row in XC.ROW_FORMS for cloud in XC.KNN_CLOUDS]


@pytest.mark.parametrize("row,cloud", FORM_CASES, ids=["%s-%s" % c for c in FORM_CASES])
def test_a_the_row_form_follows_the_addresses(pkg, row, cloud):
    """k_knn writes a row of 8 / 16 / 32 entries as 16-byte stores only where both arrays are 16-byte aligned: the launcher's
    decision ("knn_row_form") on plain buffers, on the arena's 4-byte-aligned ones and on arena buffers at multiples of 16 -- exact
    extents and guards, but the whole-row form -- and the same bits from all three"""
    t = _torch()
    ix = _handle(pkg, cloud)
    want = XC.ROW_FORMS[row]
    plain, _ = XC.run(pkg, ix, cloud, row)
    assert ix.debug_get("knn_row_form") == want, (row, cloud, "plain")
    t.cuda.synchronize()
    for aligned in (False, True):
        arena = EB.Arena(DEVICE)
        got, owned = XC.run(pkg, ix, cloud, row, arena, aligned)
        assert ix.debug_get("knn_row_form") == (want if aligned else 0), (row, cloud, aligned)
        t.cuda.synchronize()
        assert all(a % 16 == (0 if aligned else 4) for a in (arena.base + first for _n, first, _b in arena.buffers))
        arena.check((row, cloud, aligned))
        for key, a in got.items():
            mask = owned.get(key, np.zeros(len(a), bool))
            EB.Arena.untouched(a, mask, (row, cloud, key, aligned))
            assert np.array_equal(HH.bits(a)[~mask], HH.bits(plain[key])[~mask]), (row, cloud, key, aligned)


def test_a_the_bounding_box_row_is_the_numpy_box(pkg):
    """no other test pins pcpx_bounding_box_dev: its plain form against numpy, exactly"""
    got, _ = XC.run(pkg, None, "c70", "bounding_box")
    pts = HH.inputs("c1300")["points"]
    assert np.array_equal(got["box"], np.concatenate([pts.min(0), pts.max(0)]))


def test_a_some_rows_have_caller_elements_on_every_side(pkg):
    """what the masks of part a stand on: the gridded cloud leaves rows out, a slice leaves most rows out, and the slice is not empty"""
    c = XC.Buffers(pkg, _handle(pkg, "c5000g"), "c5000g")
    assert 0 < int((~c.I["inside"]).sum()) < c.n_in
    first, count = XC.slice_of(c)
    pos = XC.position_of(c)
    assert int(((pos >= first) & (pos < first + count)).sum()) == count and (pos[~c.I["inside"]] == 0xFFFFFFFF).all()


# ---- b. k_bbox's peel ---------------------------------------------------------------------------------------------------------------------
OFFSETS = (0, 4, 8, 12)
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 70, 1300)
KINDS = ("ends", "mixed")


def _peel_cloud(kind, n):
    """ends: the six extreme coordinates sit in the first three and the last three rows -- whatever is peeled in front of the first
    aligned point or left behind the last whole quad holds an extreme; mixed: rows with a NaN and with an infinity among them"""
    rng = np.random.default_rng(9000 + n)
    pts = rng.uniform(-1, 1, (n, 3)).astype(F)
    if kind == "ends" and n >= 6:
        for a in range(3):
            pts[a, a] = F(-2 - a)
            pts[n - 1 - a, a] = F(2 + a)
    if kind == "mixed" and n >= 4:
        pts[n // 2, 1] = np.nan
        pts[n - 1, 0] = np.inf
        pts[0, 2] = -np.inf
    return pts


def _reference_box(pts):
    """pcp::bounding_box: strict comparisons from +-FLT_MAX: a NaN is skipped, an infinity taken"""
    big = np.finfo(F).max
    if len(pts) == 0:
        return np.array([big] * 3 + [-big] * 3, F)
    lo = np.minimum(np.where(np.isnan(pts), F(np.inf), pts).min(0), big)
    hi = np.maximum(np.where(np.isnan(pts), F(-np.inf), pts).max(0), -big)
    return np.concatenate([lo, hi]).astype(F)


def _check_index(pkg, oracle, ix, pts, what):
    finite = np.isfinite(pts).all(1)
    assert ix.size() == int(finite.sum()), what
    if finite.any():
        assert np.array_equal(HH.bits(np.asarray(ix.bbox(), F)), HH.bits(N.finite_box(pts, finite))), what
    if len(pts) == 0:
        return
    import test_gpu_parity as TP
    k = 8
    gi, gc, gd = ix.knn_self(k, XC.EPS, want_d2=True)
    rows = np.nonzero(finite)[0]
    oi, oc, od = N.knn_over_finite(oracle, pts, finite, pts[rows], k, XC.EPS)
    TP._assert_rows_exact(pts, pts[rows], k, gi[rows], gc[rows], gd[rows], oi, oc, od)
    assert (gc[~finite] == 0).all(), what


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("kind", KINDS)
def test_b_boxes_and_builds_of_a_cloud_at_every_four_byte_offset(pkg, oracle, kind, offset):
    t = _torch()
    lib = pkg.surface._capi.load()
    arena = EB.Arena(DEVICE)
    ix = None
    try:
        for n in SIZES:
            what = (kind, offset, n)
            pts = _peel_cloud(kind, n)
            arena.take("cloud %d" % n, 3 * n, "f32", misalign=offset, data=pts)
            address = arena.address("cloud %d" % n)
            assert address % 16 == offset
            box = arena.take("box %d" % n, 6, "f32")
            t.cuda.synchronize()
            pkg.surface.check(lib.pcpx_bounding_box_dev(address, n, 0, None, box.data_ptr()))
            t.cuda.synchronize()
            got = box.cpu().numpy()
            assert np.array_equal(HH.bits(got), HH.bits(_reference_box(pts))), (what, got, _reference_box(pts))
            fresh = pkg.Index.from_device(address, n)
            try:
                _check_index(pkg, oracle, fresh, pts, what + ("create",))
            finally:
                fresh.close()
            if ix is None:
                ix = pkg.Index.from_device(address, n)
            else:
                ix.rebuild_dev(address, n)
                ix.synchronize()
            _check_index(pkg, oracle, ix, pts, what + ("rebuild",))
        t.cuda.synchronize()
        arena.check((kind, offset))
    finally:
        if ix is not None:
            ix.close()


def test_b_the_extremes_sit_in_the_peeled_head_and_in_the_tail():
    """the arithmetic of k_bbox's split, restated: at offsets 4, 8, 12 the head is 1, 2, 3 points, and for each of them 70 or 1300
    points leave a tail -- so the `ends` clouds put an extreme into both"""
    for offset in OFFSETS:
        head = ((4 - (offset // 4 & 3)) * 3) & 3
        assert (offset + 12 * head) % 16 == 0 and head == {0: 0, 4: 1, 8: 2, 12: 3}[offset]
        tails = [(n - head) % 4 for n in (70, 1300)]
        assert max(tails) > 0, offset
    pts = _peel_cloud("ends", 70)
    assert set(np.argmin(pts, 0)) <= {0, 1, 2} and set(np.argmax(pts, 0)) <= {67, 68, 69}


# ---- c. a borrowed, misaligned cloud -------------------------------------------------------------------------------------------------------
def test_c_rank_local_handles_borrow_a_cloud_four_bytes_off_a_boundary(pkg):
    t = _torch()
    dev = t.device(DEVICE)
    pts = HH.inputs("c5000")["points"]
    n, k, world = len(pts), 15, 2
    grid = np.concatenate([pts.min(0), pts.max(0)]).astype(F)
    d_plain = t.from_numpy(pts.copy()).to(dev)
    idx, cnt = t.full((n, k), -1, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int32, device=dev)
    sidx, scnt = t.full((n, k), -1, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int32, device=dev)
    arena = EB.Arena(DEVICE)
    d_pts = arena.take("borrowed cloud", 3 * n, "f32", misalign=4, data=pts)
    assert d_pts.data_ptr() % 16 == 4
    t.cuda.synchronize()
    whole = pkg.Index.from_device(d_plain.data_ptr(), n, voxel_grid=grid)
    handles = []
    try:
        whole.knn_self_dev(k, XC.EPS, idx.data_ptr(), cnt.data_ptr())
        whole.synchronize()
        covered = 0
        for rank in range(world):  # both handles live at once, both reading the caller's array
            ix = pkg.Index.from_device(d_pts.data_ptr(), n, voxel_grid=grid, shard=(rank, world), k_hint=k, borrow=True)
            handles.append(ix)
        for rank, ix in enumerate(handles):
            first, count = pkg.shard_range(ix.size(), rank, world)
            ix.knn_self_dev(k, XC.EPS, sidx.data_ptr(), scnt.data_ptr(), None, first, count)
            ix.synchronize()
            covered += count
        assert covered == n == whole.size()
        assert t.equal(scnt, cnt) and t.equal(sidx, idx)
        assert int(cnt.min()) == k
        t.cuda.synchronize()
        arena.check("borrowed cloud")
        assert d_pts.cpu().numpy().tobytes() == pts.tobytes()  # (read in place, never written)
    finally:
        for ix in handles + [whole]:
            ix.close()


def test_z_close_the_module_handles():
    for ix in _handles.values():
        ix.close()
    _handles.clear()
