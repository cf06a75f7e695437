"""CPU tests of rigid registration from correspondences (include/pcpx_register.h): the companion header as C99,
its symbols and bindings, the argument refusals (checked before any device is touched), the plan, the kernels' registers, the C++
programs of tests/cpp (register_shape.cpp compiled only, the GPU tests run it; register_refusals.cpp built and run), Horn's closed
form of csrc/pcpx_horn.h compiled for the host against an SVD, and the numpy model of the contract (tests/register_model.py) on
hand-made sets with the expected answers written out."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import register_model as M

F = np.float32
NAMES = ["pcpx_ransac_plan", "pcpx_ransac_rigid", "pcpx_ransac_rigid_dev", "pcpx_rigid_fit", "pcpx_rigid_fit_dev"]
OTHER_TABLES = ("SIGNATURES", "RADIUS_SIGNATURES", "CLUSTER_SIGNATURES", "SUBSAMPLE_SIGNATURES", "SEGMENT_SIGNATURES", "FEATURES_SIGNATURES",
                "KEYPOINTS_SIGNATURES", "DESCRIPTORS_SIGNATURES", "MATCH_SIGNATURES")
INVALID = -1
RZ90 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]


@pytest.fixture(scope="module")
def lib(pkg):
    importlib.import_module("point-cloud-processing_amd.build").build()
    return importlib.import_module("point-cloud-processing_amd._capi").load()


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcpx_register.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pcpx_[a-z0-9_]+)\s*\(", hdr)))


def test_register_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "pcpx_register.h"\n'
                   "int (*a)(uint64_t, uint64_t, uint32_t*, uint64_t*, uint64_t*) = pcpx_ransac_plan;\n"
                   "int (*b)(const float*, uint64_t, const float*, uint64_t, const uint32_t*, uint64_t, const uint64_t*, uint64_t, uint32_t, float, float,"
                   " uint32_t, int, void*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, double*, double*) = pcpx_ransac_rigid_dev;\n"
                   "int (*c)(const float*, uint64_t, const float*, uint64_t, const uint32_t*, uint64_t, uint64_t, uint32_t, float, float, uint32_t, int,"
                   " uint32_t*, uint32_t*, uint32_t*, uint32_t*, double*, double*) = pcpx_ransac_rigid;\n"
                   "int (*d)(const float*, uint64_t, const float*, uint64_t, const uint32_t*, uint64_t, const uint64_t*, const uint32_t*, uint64_t,"
                   " const uint64_t*, int, void*, double*, double*) = pcpx_rigid_fit_dev;\n"
                   "int (*e)(const float*, uint64_t, const float*, uint64_t, const uint32_t*, uint64_t, const uint32_t*, uint64_t, int, double*, double*)"
                   " = pcpx_rigid_fit;\n"
                   "int main(void){ return (a == 0) + (b == 0) + (c == 0) + (d == 0) + (e == 0) + (PCPX_RANSAC_REFIT != 1u); }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)


def test_register_symbols_exported_bound_and_disjoint(lib):
    capi = importlib.import_module("point-cloud-processing_amd._capi")
    declared = _declared()
    assert declared == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcpx_[a-z0-9_]+)", out))
    assert sorted(s for s in exported if s.startswith(("pcpx_ransac", "pcpx_rigid"))) == declared
    assert sorted(capi.REGISTER_SIGNATURES) == declared
    for table in OTHER_TABLES:
        assert not set(capi.REGISTER_SIGNATURES) & set(getattr(capi, table)), table
    for name in declared:
        assert getattr(lib, name).argtypes == capi.REGISTER_SIGNATURES[name][1]
        assert getattr(lib, name).restype == capi.REGISTER_SIGNATURES[name][0]
        assert not name.startswith(("pcpx_match", "pcpx_fpfh", "pcpx_segment", "pcpx_subsample", "pcpx_cluster"))
    assert capi.ABI_VERSION == 5 and lib.pcpx_abi_version() == 5  # pcpx.h and its ABI version stay what they were
    assert capi.PCPX_RANSAC_REFIT == 1
    pkg = importlib.import_module("point-cloud-processing_amd")
    for fn in ("ransac_plan", "ransac_rigid", "ransac_rigid_dev", "rigid_fit", "rigid_fit_dev"):
        assert callable(getattr(pkg, fn)) and fn in pkg.__all__


# ---- refusals: PCPX_ERR_INVALID before any device is touched (this machine may have none) ------------------------------------------------
def _ransac(lib, dev_form, p=1, np_=8, q=1, nq=8, pairs=1, cap=8, T=64, tau2=0.01, s2=0.81, flags=0, found=1, refit=0):
    a = np.zeros(64, F)
    pr = np.zeros(64, np.uint32)
    o = np.full(4, 9, np.uint32)
    x = np.zeros(16)
    ptr = lambda on, arr: arr.ctypes.data_as(C.c_void_p) if on else None
    if dev_form:
        st = lib.pcpx_ransac_rigid_dev(ptr(p, a), np_, ptr(q, a), nq, ptr(pairs, pr), cap, None, T, 1, tau2, s2, flags, 0, None, ptr(found, o), None, None,
                                       None, None, None, ptr(refit, x))
    else:
        st = lib.pcpx_ransac_rigid(ptr(p, a), np_, ptr(q, a), nq, ptr(pairs, pr), cap, T, 1, tau2, s2, flags, 0, ptr(found, o), None, None, None, None,
                                   ptr(refit, x))
    assert o.tolist() == [9] * 4  # (a refused call writes nothing)
    return st


def _fit(lib, dev_form, p=1, np_=8, q=1, nq=8, pairs=1, cap=8, pos=1, npos=8, out=1):
    a = np.zeros(64, F)
    pr = np.zeros(64, np.uint32)
    x = np.zeros(16)
    ptr = lambda on, arr: arr.ctypes.data_as(C.c_void_p) if on else None
    if dev_form:
        return lib.pcpx_rigid_fit_dev(ptr(p, a), np_, ptr(q, a), nq, ptr(pairs, pr), cap, None, ptr(pos, pr), npos, None, 0, None, ptr(out, x), None)
    return lib.pcpx_rigid_fit(ptr(p, a), np_, ptr(q, a), nq, ptr(pairs, pr), cap, ptr(pos, pr), npos, 0, ptr(out, x), None)


@pytest.mark.parametrize("dev_form", [False, True])
def test_register_argument_refusals(lib, dev_form):
    big = 0xFFFFFFFF
    for bad in (dict(p=0), dict(q=0), dict(pairs=0), dict(T=0), dict(T=big), dict(T=2 ** 40), dict(cap=big), dict(cap=2 ** 33), dict(np_=2 ** 32),
                dict(nq=2 ** 32), dict(flags=2), dict(flags=0x80000001), dict(flags=1, refit=0), dict(found=0)):
        assert _ransac(lib, dev_form, **bad) == INVALID, bad
        assert lib.pcpx_last_error(), bad
    for tau2 in (-1e-30, -1.0, float("nan"), float("-inf")):
        assert _ransac(lib, dev_form, tau2=tau2) == INVALID, tau2
        assert b"max_distance_sq" in lib.pcpx_last_error()
    for s2 in (-0.5, 1.0000001, float("nan"), float("inf")):
        assert _ransac(lib, dev_form, s2=s2) == INVALID, s2
        assert b"edge_similarity_sq" in lib.pcpx_last_error()
    for bad in (dict(p=0), dict(q=0), dict(pairs=0), dict(cap=big), dict(npos=big), dict(pos=0), dict(out=0), dict(np_=2 ** 32)):
        assert _fit(lib, dev_form, **bad) == INVALID, bad
        assert lib.pcpx_last_error(), bad


def _plan(lib, T, cap):
    s, r, b = C.c_uint32(9), C.c_uint64(9), C.c_uint64(9)
    assert lib.pcpx_ransac_plan(T, cap, C.byref(s), C.byref(r), C.byref(b)) == 0, lib.pcpx_last_error()
    return s.value, r.value, b.value


def test_ransac_plan(lib):
    for bad in ((0, 10), (0xFFFFFFFF, 10), (10, 0xFFFFFFFF)):
        assert lib.pcpx_ransac_plan(*bad, None, None, None) == INVALID, bad
    assert lib.pcpx_ransac_plan(5, 5, None, None, None) == 0  # every output is optional
    rng = np.random.default_rng(1)
    sizes = [(1, 0), (1, 1), (64, 100), (65, 100000), (1000, 1000000), (10 ** 6, 10 ** 4), (4 * 10 ** 6, 1000), (1, 2 ** 32 - 2), (2 ** 32 - 2, 1)]
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(1, 500000, 40), rng.integers(1, 300000, 40))]
    for T, cap in sizes:
        seg, rows, scratch = _plan(lib, T, cap)
        if cap == 0:
            assert seg == 0 and rows == 0
        else:
            assert seg >= 1 and rows % 256 == 0 and (seg - 1) * rows < cap <= seg * rows, (T, cap, seg, rows)
            groups = -(-T // 64)
            assert seg <= max(1, min(256, -(-16384 // groups), cap // 256)), (T, cap, seg)  # about 16 384 waves, segments of 256 rows at the least
        assert seg <= 256
        assert scratch % 256 == 0 and scratch >= 32 * cap + 4 * T * seg  # (the records and the counts are part of it)
    # few hypotheses are split, so that the call fills the device; many need not be
    assert _plan(lib, 64, 65536)[:2] == (256, 256) and _plan(lib, 10 ** 5, 1000)[:2] == (2, 512) and _plan(lib, 10 ** 6, 10 ** 4)[:2] == (2, 5120)
    assert _plan(lib, 4 * 10 ** 6, 1000)[0] == 1 and _plan(lib, 64, 100)[0] == 1
    # the scratch grows with either size
    for fixed in (1, 1000, 100000):
        by_T = [_plan(lib, T, fixed)[2] for T in (1, 64, 65, 4096, 10 ** 5, 10 ** 6)]
        by_C = [_plan(lib, fixed, cap)[2] for cap in (0, 1, 255, 256, 257, 1000, 10 ** 4, 10 ** 6)]
        assert by_T == sorted(by_T) and by_C == sorted(by_C), (fixed, by_T, by_C)
    # 2 and 3 segments with the last one a single row, full, and one row short: the shapes tests/test_gpu_register.py runs
    found = set()
    for cap in range(1, 2100):
        seg, rows, _b = _plan(lib, 4096, cap)
        last = cap - (seg - 1) * rows
        if seg in (2, 3):
            found |= {(seg, "one")} if last == 1 else {(seg, "full")} if last == rows else {(seg, "short")} if last == rows - 1 else set()
    assert found == {(s, k) for s in (2, 3) for k in ("one", "full", "short")}, found


@pytest.mark.timeout(600)
def test_register_kernels_use_no_scratch_and_spill_nothing():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "pcpx_register.hip", "k_"],
                         capture_output=True, text=True, timeout=580, check=True).stdout
    rows = dict((m[0], [int(v) for v in m[1:]]) for m in re.findall(
        r"(k_\w+(?:<[^>]*>)?)\(.*?vgpr\s+(\d+) sgpr\s+(\d+) sspill\s+(\d+) vspill\s+(\d+) scratch\s+(\d+) lds\s+(\d+)", out))
    assert len(out.strip().splitlines()) == len(rows), out  # (every kernel of the file is among them)
    own = sorted(set(re.sub(r"<.*", "", name) for name in rows if not name.startswith("k_scan_")))
    assert own == ["k_fit_solve", "k_fixed_final", "k_fixed_partial", "k_ransac_best", "k_ransac_count", "k_ransac_emit", "k_reg_compact", "k_reg_pack"], out
    for name, (vgpr, sgpr, sspill, vspill, scratch, lds) in rows.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, out)
        assert lds == 0 or name.startswith(("k_scan_", "k_fixed_partial")), (name, out)  # (the scan's and the fit's block sums)
        assert vgpr <= 128 and sgpr <= 102, (name, out)
    assert rows["k_ransac_count"][5] == 0 and rows["k_ransac_count"][0] <= 64, out  # no LDS, and eight waves a SIMD by its vector registers


def test_cpp_register_program_compiles(tmp_path, pkg):
    inc = os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", os.path.join(ROOT, "tests", "cpp", "register_shape.cpp"),
                    "-o", str(tmp_path / "register_shape.o")], check=True)


def test_cpp_refusals_program_runs_without_a_device(tmp_path, lib):
    capi = importlib.import_module("point-cloud-processing_amd._capi")
    inc, pkgdir = os.path.join(ROOT, "include"), os.path.dirname(capi.LIB_PATH)
    exe = str(tmp_path / "register_refusals")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, os.path.join(ROOT, "tests", "cpp", "register_refusals.cpp"),
                    "-o", exe, "-L", pkgdir, "-lpcpx", "-Wl,-rpath," + pkgdir, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "0 checks failed" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# ---- Horn's closed form, compiled for the host ------------------------------------------------------------------------------------------
def _kabsch(p, q):
    """float64 SVD Kabsch with the determinant correction: (R, t) minimising sum |R p + t - q|^2"""
    pbar, qbar = p.mean(0), q.mean(0)
    U, _s, Vt = np.linalg.svd((p - pbar).T @ (q - qbar))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, qbar - R @ pbar


def test_horn_rotation_on_the_host_equals_the_svd(tmp_path):
    src = tmp_path / "horn.cpp"
    src.write_text('#include "pcpx_horn.h"\n#include <cstdio>\n'
                   "int main(){ double h[9], r[9]; while (std::scanf(\"%la %la %la %la %la %la %la %la %la\", h, h+1, h+2, h+3, h+4, h+5, h+6, h+7, h+8) == 9) {"
                   " pcpx::horn_rotation(h, r); for (int i = 0; i < 9; ++i) std::printf(\"%a \", r[i]); std::printf(\"\\n\"); } return 0; }\n")
    exe = str(tmp_path / "horn")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I",
                    os.path.join(ROOT, "point-cloud-processing_amd", "csrc"), str(src), "-o", exe], check=True)
    rng = np.random.default_rng(3)
    cases = []
    for i in range(40):
        p = rng.normal(size=(50, 3)) * rng.uniform(0.1, 10, 3)
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        A *= np.sign(np.linalg.det(A)) if i % 4 else -np.sign(np.linalg.det(A))  # every fourth set is mirrored
        q = p @ A.T + rng.normal(0, 0.01, p.shape)
        cases.append((p - p.mean(0), q - q.mean(0)))
    Hs = [p.T @ q for p, q in cases] + [np.zeros((3, 3)), np.eye(3), -np.eye(3)]
    text = "\n".join(" ".join(float(v).hex() for v in H.reshape(9)) for H in Hs) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    for i, H in enumerate(Hs):
        R = np.array([float.fromhex(v) for v in out[i].split()]).reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14, i  # always a proper rotation
        if i < len(cases):
            val = np.sort(np.linalg.eigvalsh(M.horn_matrix(H)))
            gap = (val[-1] - val[-2]) / np.abs(val).max()
            assert gap >= 0.1 or i % 4 == 0, (i, gap)  # (a mirrored set's best rotation is less sharply defined)
            assert np.abs(R - _kabsch(*cases[i])[0]).max() <= 1e-13 / gap, (i, gap)
    assert np.array_equal(np.array([float.fromhex(v) for v in out[len(cases)].split()]).reshape(3, 3), np.eye(3))  # H = 0: the identity
    assert np.array_equal(np.array([float.fromhex(v) for v in out[len(cases) + 1].split()]).reshape(3, 3), np.eye(3))


# ---- the model on hand-made sets ------------------------------------------------------------------------------------------------------
def _fmix32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_model_sampling_is_the_written_formula():
    for seed, C_ in ((0, 3), (0x1234, 1000), (0xFFFFFFFF, 2 ** 32 - 2), (7, 1)):
        hs = [0, 1, 2, 63, 64, 4095, 2 ** 32 - 2]
        got = M.slots(np.array(hs, np.uint64), seed, C_)
        for h, row in zip(hs, got.tolist()):
            w = _fmix32_int(h ^ seed)
            assert row == [(_fmix32_int((w + (s + 1) * 0x9E3779B9) & 0xFFFFFFFF) * C_) >> 32 for s in range(3)]
            assert all(0 <= v < C_ for v in row)
    assert M.slots(np.array([5], np.uint64), 9, 1000).tolist() != M.slots(np.array([5], np.uint64), 10, 1000).tolist()


def _rz90(p, shift):
    p = np.asarray(p, F)
    return np.stack([-p[:, 1], p[:, 0], p[:, 2]], 1) + np.asarray(shift, F)


def test_model_quarter_turn_of_grid_points_is_exact():
    # an axis-parallel right angle with power-of-two legs: every square root and division is exact
    p = np.array([[1, 1, 1], [3, 1, 1], [1, 5, 1]], F) / F(128)
    q = _rz90(p, [0.5, -0.25, 2])
    x = np.concatenate([p, q], 1)
    R, t, ok = M.pose_of(x[0], x[1], x[2], 0.81)
    assert ok.tolist() == [True] and R[0].tolist() == RZ90
    assert t[0].tolist() == [0.5, -0.25, 2.0]
    # scored against itself and two others: the three are inliers at tau = 0, a moved target is not
    rec = np.concatenate([x, [[0.25, 0.5, 0.75, -0.5 + 0.5, 0.25 - 0.25, 0.75 + 2]], [[0.25, 0.5, 0.75, 0, 0, 0]]]).astype(F)
    assert M.inlier_mask(R, t, rec, 0.0).tolist() == [[True, True, True, True, False]]
    assert M.scores(R, t, rec, 0.0).tolist() == [4]
    # the float64 transform with origins: R widened, t_abs = (o_q + t) - R o_p
    o = np.array([2, 4, 8, 16, 32, 64], F)
    assert M.transform64(R[0], t[0], o).tolist() == [0, -1, 0, 16 + 0.5 + 4, 1, 0, 0, 32 - 0.25 - 2, 0, 0, 1, 64 + 2 - 8, 0, 0, 0, 1]


def test_model_repeated_slots_make_a_hypothesis_invalid():
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0]], F)
    pairs = np.array([[0, 0], [1, 1], [2, 2]], np.uint32)
    rec, origins = M.records(p, _rz90(p, [1, 1, 1]), pairs)
    assert origins.tolist() == [0, 0, 0, 1, 1, 1] and rec[:, 3:].tolist() == [[0, 0, 0], [0, 2, 0], [-4, 0, 0]]
    hs = np.arange(600, dtype=np.uint64)
    sl = M.slots(hs, 5, 3)
    distinct = np.array([len(set(r)) == 3 for r in sl.tolist()])
    _R, _t, valid = M.hypotheses(rec, hs, 5, 0.0)
    assert np.array_equal(valid, distinct) and 60 < distinct.sum() < 220  # (6 of the 27 triples are permutations)
    res = M.ransac(p, _rz90(p, [1, 1, 1]), pairs, 600, 5, 0.0, 0.0)
    found, h, score, inl, xf = res.best_of(600)
    assert (found, h, score, inl.tolist()) == (1, int(np.argmax(distinct)), 3, [0, 1, 2])  # all valid ones tie at 3: the lowest h
    assert np.allclose(xf.reshape(4, 4), [[0, -1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]], atol=1e-6)
    assert M.ransac(p, p, pairs[:2], 64, 5, 1.0, 0.0).best_of(64)[:3] == (0, 0, 0)  # C < 3: nothing is valid


def test_model_collinear_triple_and_bad_records_are_invalid():
    line = np.array([[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [3, 3, 3, 3, 3, 3]], F)
    assert M.pose_of(line[0], line[1], line[2], 0.0)[2].tolist() == [False]  # c = a x b = 0
    tri = np.array([[0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 2, 0], [0, 4, 0, -4, 0, 0]], F)
    assert M.pose_of(tri[0], tri[1], tri[2], 1.0)[2].tolist() == [True]
    assert M.pose_of(tri[0], tri[0], tri[2], 0.0)[2].tolist() == [False]  # a = 0
    nan_rec = np.array([np.nan, 0, 0, 0, 0, 0], F)
    for where in range(3):
        x = [tri[0], tri[1], tri[2]]
        x[where] = nan_rec
        assert M.pose_of(*x, 0.0)[2].tolist() == [False], where
    # records: an index out of range, a NaN and an inf coordinate become the NaN record, and never count as inliers
    P = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0], [np.nan, 0, 0], [1, 1, np.inf]], F)
    pairs = np.array([[0, 0], [1, 1], [2, 2], [3, 1], [1, 4], [5, 0], [0, 5]], np.uint32)
    rec, _o = M.records(P, P, pairs)
    assert np.isnan(rec[:, 0]).tolist() == [False, False, False, True, True, True, True] and not rec[3:, 1:].any()
    R, t, _ok = M.pose_of(rec[0], rec[1], rec[2], 0.0)
    assert M.inlier_mask(R, t, rec, np.inf).tolist() == [[True, True, True, False, False, False, False]]
    # correspondence 0 not usable: the origins are zero
    rec2, o2 = M.records(P, P, pairs[::-1])
    assert o2.tolist() == [0] * 6 and rec2[4].tolist() == [0, 4, 0, 0, 4, 0]


def test_model_edge_gate_rejects_a_stretched_triangle():
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0]], F)
    x = np.concatenate([p, F(2) * p], 1)  # the target triangle is twice as large: every squared edge is four times its partner
    assert M.pose_of(x[0], x[1], x[2], 0.0)[2].tolist() == [True]
    assert M.pose_of(x[0], x[1], x[2], 0.25)[2].tolist() == [True]  # Lp >= 0.25 Lq holds with equality
    assert M.pose_of(x[0], x[1], x[2], float(np.nextafter(F(0.25), F(1))))[2].tolist() == [False]
    assert M.pose_of(x[0], x[1], x[2], float(F(0.9) * F(0.9)))[2].tolist() == [False]
    # only the third edge is off: x2 moved along the hypotenuse's normal keeps la2, changes lb2 and ld2
    y = x.copy()
    y[:, 3:] = x[:, :3]
    y[2, 3:] = [0, 5, 0]
    assert M.pose_of(y[0], y[1], y[2], 0.5)[2].tolist() == [True] and M.pose_of(y[0], y[1], y[2], 0.81)[2].tolist() == [False]


def test_model_rigid_fit_matches_the_svd_and_is_proper_for_a_mirrored_set():
    rng = np.random.default_rng(8)
    P = rng.uniform(-1, 1, (300, 3)).astype(F)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A *= np.sign(np.linalg.det(A))
    Q = (P @ A.T + [0.5, 1, -2] + rng.normal(0, 0.01, P.shape)).astype(F)
    pairs = np.stack([np.arange(300), np.arange(300)], 1).astype(np.uint32)
    xf, rms = M.rigid_fit(P, Q, pairs)
    R, t = _kabsch(P.astype(np.float64), Q.astype(np.float64))
    assert np.abs(xf.reshape(4, 4)[:3, :3] - R).max() <= 1e-12 and np.abs(xf.reshape(4, 4)[:3, 3] - t).max() <= 1e-12
    assert 0.01 < rms < 0.03
    pos = np.array([5, 7, 9, 200, 299, 300, 4000], np.uint32)  # (positions beyond the count are not usable)
    xf2, _ = M.rigid_fit(P, Q, pairs, pos)
    R2, t2 = _kabsch(P[pos[:5]].astype(np.float64), Q[pos[:5]].astype(np.float64))
    assert np.abs(xf2.reshape(4, 4)[:3, :3] - R2).max() <= 1e-11
    xm, _ = M.rigid_fit(P, Q * F(-1), pairs)
    Rm = xm.reshape(4, 4)[:3, :3]
    assert abs(np.linalg.det(Rm) - 1) <= 1e-12 and np.abs(Rm - _kabsch(P.astype(np.float64), -Q.astype(np.float64))[0]).max() <= 1e-10
    ident, nan = M.rigid_fit(P, Q, pairs[:2])
    assert ident.tolist() == np.eye(4).reshape(16).tolist() and np.isnan(nan)
