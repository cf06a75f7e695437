"""The C++17 drop-in headers (include/pcp/): compile the reference-style scenarios of
tests/cpp/test_pcp_api.cpp against them with g++ and link libpcpx.so (CPU); run them (GPU)."""
import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "point-cloud-processing_amd")


@pytest.fixture(scope="module")
def binary(tmp_path_factory, pkg):
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    out = tmp_path_factory.mktemp("cpp") / "test_pcp_api"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_pcp_api.cpp"), "-o", str(out), "-L", PKG, "-lpcpx",
           "-Wl,-rpath," + PKG, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"]
    subprocess.run(cmd, check=True)
    return str(out)


def test_headers_compile_and_link(binary):
    assert subprocess.run([binary, "--compile-only"]).returncode == 0


def test_every_public_header_is_self_contained(tmp_path):
    inc = os.path.join(ROOT, "include")
    for dp, _, files in os.walk(os.path.join(inc, "pcp")):
        for f in files:
            rel = os.path.relpath(os.path.join(dp, f), inc)
            src = tmp_path / "t.cpp"
            src.write_text('#include "%s"\nint main() { return 0; }\n' % rel)
            subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src)], check=True)


def _compile(tmp_path, source, name, extra=()):
    out = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), *extra,
           os.path.join(ROOT, "tests", "cpp", source), "-o", str(out), "-L", PKG, "-lpcpx", "-Wl,-rpath," + PKG,
           "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"]
    subprocess.run(cmd, check=True)
    return str(out)


def test_cpp_ply_reader_and_writer(tmp_path, pkg):
    """include/pcp/io/ply.hpp: the bunny data file, the three formats, the failure cases."""
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "test_ply_io.cpp", "test_ply_io")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # the C++ and Python readers agree on the data file, and each reads what the other writes
    pts, _ = pkg.ply.read_ply(os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply"))
    first = [float(x) for x in r.stdout.split("first (")[1].split(")")[0].split()]
    assert [float("%.9g" % v) for v in pts[0]] == first
    for i in (0, 1, 2):
        rp, rn = pkg.ply.read_ply(str(tmp_path / ("rt%d.ply" % i)))
        assert rp.shape == (3, 3) and rn.shape == (2, 3) and abs(rn[1, 2] - 0.8) < 1e-6


def test_containers_from_large_ranges(tmp_path, pkg):
    """include/pcp/gpu/host_capture.hpp: the constructors' multi-threaded walk over a large range gives the container the
    one-by-one insertion gives (elements, order, out-of-grid drop, coordinates, boxes).  Host only -- no query, no device."""
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "test_host_capture.cpp", "test_host_capture")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host capture: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_kdtree_in_one_to_sixteen_dimensions(tmp_path, pkg):
    """basic_linked_kdtree_t<Element, K, Map> for K = 1, 2, 3 (the device index) and 4, 5, 8, 16 (pcpx_kd_*) -- the reference is generic in K, include/pcp/kdtree/linked_kdtree.hpp:64:
    k nearest neighbours, box ranges and aabb() against brute force on the host (tests/cpp/test_kdtree_dims.cpp)."""
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "test_kdtree_dims.cpp", "test_kdtree_dims")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_curve_key_is_a_continuous_bijection(tmp_path):
    """csrc/pcpx_curve.h compiled for the host with hipcc (no GPU needed): the Hilbert index the index is sorted by."""
    exe = tmp_path / "test_curve"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "test_curve.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "curve key: ok" in r.stdout, r.stdout


@pytest.mark.gpu
def test_reference_scenarios_through_cpp_headers(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all scenarios passed" in r.stdout


@pytest.mark.gpu
def test_unchanged_reference_program_shape(tmp_path, pkg, bunny_golden):
    """examples/simple_example.cpp:6-110 call for call (plain lambda knn map, per-point range_search, read/write PLY)
    against the drop-in headers, checked against the bunny's golden rows; prints the per-phase times."""
    import importlib
    import json
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "simple_example_shape.cpp", "simple_example_shape")
    gdir = tmp_path / "golden"
    gdir.mkdir()
    for key in ("query_index", "knn_idx", "normals", "range_count_r001"):
        bunny_golden[key].tofile(str(gdir / (key + ".bin")))
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply"), str(tmp_path / "out.ply"), str(gdir)],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["golden_rows_checked"] == 512 and res["points"] == 35947
    # the per-point loops are served from batched launches: far from one GPU round trip per point
    assert res["estimate_normals_ms"] < 2000 and res["density_loop_ms"] < 2000
    pts, nrm = pkg.ply.read_ply(str(tmp_path / "out.ply"))
    assert pts.shape == (35947, 3) and nrm.shape == (35947, 3)


def test_normals_estimation_example_compiles(tmp_path):
    """Every pcp call shape of examples/normals_estimation.cpp (tests/cpp/normals_estimation_shape.cpp) builds against the
    drop-in headers with -Wall -Wextra -Werror (CPU: compile and link only)."""
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    assert os.path.exists(_compile(tmp_path, "normals_estimation_shape.cpp", "normals_estimation_shape"))


@pytest.mark.gpu
def test_normals_estimation_example_shape(tmp_path, pkg, oracle):
    """That program run on the bunny without and with the bilateral step (k = 15, 2 iterations, sigmaf = 2 x and
    sigmag = 0.5 x the mean neighbour distance): normals, their orientation and the filtered normals equal what the batched
    Python entry points give for the same parameters."""
    import importlib
    import json
    import numpy as np
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "normals_estimation_shape.cpp", "normals_estimation_shape")
    src = os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply")
    r = subprocess.run([exe, src, str(tmp_path / "plain.ply"), "15", "seq"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe, src, str(tmp_path / "out.ply"), "15", "par", "2", "2.0", "0.5"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["points"] == 35947 and res["unit_normals"] == 35947
    # (the reference applies the filter's Jacobian itself, not its inverse transpose, to the normal -- bilateral_filter.hpp:254-265:
    # "should be used only for point rendering" -- so the filtered field is far from the input one; nothing is asserted about that)
    assert res["estimate_normals_ms"] < 2000 and res["orientation_ms"] < 4000 and res["bilateral_ms"] < 2000
    pts, plain = pkg.ply.read_ply(str(tmp_path / "plain.ply"))
    _, filtered = pkg.ply.read_ply(str(tmp_path / "out.ply"))
    tree = pkg.LinkedKdTree(pts)
    oriented = tree.oriented_normals_knn_self(15)[0]
    cos = np.sum(plain * oriented, axis=1)
    assert np.mean(cos > 1 - 1e-4) > 0.999, float(np.mean(cos > 1 - 1e-4))
    avg = float(np.mean(tree.mean_knn_distance_self(15), dtype=np.float32))
    assert abs(avg - res["mean_distance"]) <= 1e-5 * avg  # (a float mean in another order)
    expect = pkg.bilateral_filter_normals(pts, plain, 2.0 * res["mean_distance"], 0.5 * res["mean_distance"], K=2)
    assert np.sum(filtered * expect, axis=1).min() > 1 - 1e-6
    ref = oracle.bilateral_filter_normals(pts, plain, 2.0 * res["mean_distance"], 0.5 * res["mean_distance"], K=2, nthreads=8)
    close = np.sum(filtered.astype(np.float64) * ref, axis=1) > 1 - 1e-4
    print("rows within 1e-4 cosine of the oracle: %.5f" % float(np.mean(close)))
    assert np.mean(close) > 0.99


def test_density_filter_example_compiles(tmp_path):
    """Every pcp call shape of examples/filter_point_cloud_noise_by_density.cpp (tests/cpp/density_filter_shape.cpp, including
    pcp/common/timer.hpp) builds against the drop-in headers (CPU: compile and link only)."""
    import importlib
    importlib.import_module("point-cloud-processing_amd.build").build()
    assert os.path.exists(_compile(tmp_path, "density_filter_shape.cpp", "density_filter_shape"))


@pytest.mark.gpu
def test_density_filter_example_shape(tmp_path, pkg):
    """The same program on the bunny (threshold 12, multiplier 1, k = 15): its radius is the mean of the mean neighbour
    distances, and the points it keeps are exactly those whose ball holds at least `threshold` points."""
    import importlib
    import json
    import numpy as np
    importlib.import_module("point-cloud-processing_amd.build").build()
    exe = _compile(tmp_path, "density_filter_shape.cpp", "density_filter_shape")
    src = os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply")
    r = subprocess.run([exe, src, str(tmp_path / "out.ply"), "12", "1", "15"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    pts, _ = pkg.ply.read_ply(src)
    tree = pkg.LinkedOctree(pts)
    mean = float(np.mean(tree.mean_knn_distance_self(15), dtype=np.float32))
    assert abs(mean - res["radius"]) <= 1e-5 * mean
    keep = tree.range_count_self(np.float32(res["radius"])) >= 12
    assert res["points_before"] == len(pts) and res["points_after"] == int(keep.sum())
    assert 0 < res["points_after"] < len(pts)
    out, _ = pkg.ply.read_ply(str(tmp_path / "out.ply"))
    assert np.array_equal(out, pts[keep])  # remove_if keeps the survivors in order
    assert res["radius_ms"] < 2000 and res["filter_ms"] < 2000
