"""Every entry point from eight host threads at once (tests/host_threads.py has the plans, the threads and the counting; what the
plans promise is proved on the CPU in tests/test_host_threads_cpu.py): the promises of include/pcpx.h, Conventions, "Threads".

  A  own handles on own streams, every row of tests/exact_buffers_cases.py on arrays of the thread's stream
  B  one shared handle per home cloud, every row of tests/handle_history_cases.py through its `run`, with rebuilds in between
  C  handle churn: create from host memory, one row, close, six times per thread
  D  (inside A and B) a refused call per thread and its error text; the current device where there are two devices

Each part comes as two tests: the baselines on the main thread with nothing else running -- which also fill the Python-side caches,
so that no thread does -- and the threads.  Every comparison is of bits with those baselines.  A part prints its overlap count and
asserts that it is positive.  Measured on an MI355X (one device visible: the current-device check of part D was skipped there;
the counts change a little from run to run):

    part   baselines          threads   library calls   began with another thread inside
    A      129 in 0.71 s      0.08 s    718             579
    B       44 in 0.04 s      0.03 s    264             228
    C        2 in 0.00 s      0.03 s    312             277

(This module alone, so part A's test of baselines took 2.1 s with the first use of the device and every other test under 0.2 s.
Behind the rest of the suite the baselines took 0.05 s, part A's threads 0.15 s with 513 of 718 calls overlapping, B's 0.04 s with
225 of 264, C's 0.03 s with 285 of 312.)

Nothing is compared with a tolerance and no shape is new: the tables' clouds c70, c1300, c5000, c5000g and c33000."""
import threading
import time

import pytest

import exact_buffers_cases as XC
import handle_history_cases as HH
import host_threads as HT

pytestmark = pytest.mark.gpu

_base = {}     # part -> {case: the outputs}
_seconds = {}  # part -> wall seconds its baselines took
_main = {}     # the main thread's stream and handles (part A's baselines)


def _torch():
    return pytest.importorskip("torch")


def _say(*what):
    print(*what, flush=True)


def _capi(pkg):
    return pkg.surface._capi


def _names(pkg):
    capi = _capi(pkg)
    return [name for key, table in vars(capi).items() if key.endswith("SIGNATURES") for name in table]  # (every function that load() declares)


def _guarded(what, fn):
    """fn() on the main thread; a HIP error ends the session: nothing more is started on a device that may have faulted"""
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        pytest.exit("%s: %s: %s" % (what, type(e).__name__, e), returncode=3)


def _threads(pkg, part, plan, act, first=None, last=None, two_devices=False):
    """the part's threads under the watch; ends the session on a hang or a HIP error, else returns (outcome, watch)"""
    t = _torch()
    limit = HT.limit_for(_seconds[part])
    lib = _capi(pkg).load()
    t.cuda.synchronize()
    with HT.Watch(lib, _names(pkg), current_device=t.cuda.current_device if two_devices else None) as watch:
        _say("part %s: %d steps, %d threads, limit %.0f s (baselines %.2f s)" % (part, len(plan), HT.T, limit, _seconds[part]))
        out = HT.run_plan(plan, act, limit, first=lambda i: first(i, watch) if first else None, last=last)
    _say("part %s: %.2f s, %d library calls, %d began while another thread's call was inside the library"
         % (part, out.seconds, watch.calls, watch.overlapped))
    if out.hung or out.fatal:
        pytest.exit("part %s: %s" % (part, "; ".join(out.fatal) or "no return within %.0f s: %s" % (limit, out.hung)), returncode=3)
    t.cuda.synchronize()
    return out, watch


def _conclude(part, out, watch):
    assert not out.failures, (part, len(out.failures), out.failures[:6])
    assert not watch.moved, (part, watch.moved[:6])
    assert watch.overlapped > 0, "part %s: no call began while another thread was inside the library: nothing was tested" % part


def _new_handle(pkg, cloud, stream_handle):
    ix = pkg.Index.from_device(HH.on_device(cloud).data_ptr(), HH.SIZES[cloud], stream=stream_handle, voxel_grid=HH.GRID if HH.gridded(cloud) else None)
    assert ix.size() == int(HH.inputs(cloud)["inside"].sum())
    return ix


def _refuse(pkg, ix, i, d_counts, out):
    capi = _capi(pkg)
    for message in HT.refused_call(capi.load(), capi, ix, i, d_counts.data_ptr()):
        out.failed("part D", message)


# ---- A --------------------------------------------------------------------------------------------------------------------------------
def test_a0_baselines_on_the_main_thread(pkg):
    t = _torch()
    t0 = time.perf_counter()

    def make():
        _main["stream"] = t.cuda.Stream(device=t.device("cuda", 0))
        for cloud in XC.CLOUDS:
            _main[cloud] = _new_handle(pkg, cloud, _main["stream"].cuda_stream)
        base = {}
        for row in XC.ROWS:
            for cloud in XC.clouds_of(row):
                base[(row, cloud)] = XC.run(pkg, None if XC.ROWS[row].family == "free" else _main[cloud], cloud, row)[0]
                t.cuda.synchronize()
        return base
    _base["A"] = _guarded("part A, baselines", make)
    _seconds["A"] = time.perf_counter() - t0
    _say("part A: %d baselines in %.2f s" % (len(_base["A"]), _seconds["A"]))
    assert len(_base["A"]) == sum(len(XC.clouds_of(r)) for r in XC.ROWS)


def test_a1_own_handles_on_own_streams(pkg):
    t = _torch()
    if "A" not in _base:
        test_a0_baselines_on_the_main_thread(pkg)
    base = _base["A"]

    def first(i, watch):
        stream = t.cuda.Stream(device=t.device("cuda", 0))
        handles = {cloud: _new_handle(pkg, cloud, stream.cuda_stream) for cloud in XC.CLOUDS}  # (eight builds side by side)
        with t.cuda.stream(stream):
            counts = t.full((HH.SIZES["c70"],), HH.FILL, dtype=t.int32, device=t.device("cuda", 0))
        stream.synchronize()
        return stream, handles, counts

    def act(i, ctx, action, out):
        stream, handles, counts = ctx
        if action[0] == "fail":
            return _refuse(pkg, handles["c70"], i, counts, out)
        row = action[1]
        for cloud in XC.clouds_of(row):
            got = HT.run_threaded(pkg, None if XC.ROWS[row].family == "free" else handles[cloud], cloud, row, stream)
            for message in HT.differing_bits(got, base[(row, cloud)]):
                out.failed("A", row, cloud, "thread %d" % i, message)

    def last(i, ctx):
        stream, handles, _counts = ctx
        for ix in handles.values():
            ix.close()
        stream.synchronize()
    _conclude("A", *_threads(pkg, "A", HT.plan_a(), act, first, last))


def test_a2_close_the_main_handles():
    for cloud in XC.CLOUDS:
        if cloud in _main:
            _main.pop(cloud).close()
    _torch().cuda.synchronize()


# ---- B, C: the baselines are handle_history_cases.fresh --------------------------------------------------------------------------------
def _fresh_baselines(pkg, part, cases):
    t = _torch()
    t0 = time.perf_counter()

    def make():
        base = {(cloud, row): HH.fresh(pkg, cloud, row) for cloud, row in cases}
        for cloud in HT.shared_clouds():
            HH.on_device(cloud)  # (what a rebuild reads)
        t.cuda.synchronize()
        return base
    _base[part] = _guarded("part %s, baselines" % part, make)
    _seconds[part] = time.perf_counter() - t0
    _say("part %s: %d baselines in %.2f s" % (part, len(_base[part]), _seconds[part]))


def test_b0_baselines_on_the_main_thread(pkg):
    _fresh_baselines(pkg, "B", [(HT.home_of(row), row) for row in HH.ROWS])
    assert len(_base["B"]) == len(HH.ROWS)


def test_b1_one_shared_handle_per_home_cloud(pkg):
    t = _torch()
    if "B" not in _base:
        test_b0_baselines_on_the_main_thread(pkg)
    base = _base["B"]
    two_devices = pkg.device_count() >= 2
    _say("part D: %d device(s): the current-device check %s" % (pkg.device_count(), "runs on the odd threads" if two_devices else "is skipped"))
    shared = _guarded("part B, the shared handles", lambda: {cloud: HH.build(pkg, cloud) for cloud in HT.shared_clouds()})
    counts = t.full((HH.SIZES["c5000g"],), HH.FILL, dtype=t.int32, device=t.device("cuda", 0))
    t.cuda.synchronize(0)

    def first(i, watch):
        if two_devices and i % 2 == 1:
            t.cuda.set_device(1)
            watch.expect[threading.get_ident()] = 1

    def act(i, ctx, action, out):
        if action[0] == "fail":
            return _refuse(pkg, shared["c5000g"], i, counts, out)
        if action[0] == "rebuild":
            return HH.rebuild(shared[action[1]], action[1])
        row = action[1]
        cloud = HT.home_of(row)
        got = HH.run(pkg, None if HT.family_b(row) == "free" else shared[cloud], cloud, row)
        for message in HT.differing(got, base[(cloud, row)]):
            out.failed("B", row, cloud, "thread %d" % i, message)
    try:
        _conclude("B", *_threads(pkg, "B", HT.plan_b(), act, first, two_devices=two_devices))
    finally:
        for ix in shared.values():
            ix.close()
        t.cuda.synchronize(0)


def test_c0_baselines_on_the_main_thread(pkg):
    _fresh_baselines(pkg, "C", HT.CHURN_CASES)


def test_c1_handle_churn(pkg):
    if "C" not in _base:
        test_c0_baselines_on_the_main_thread(pkg)
    base = _base["C"]

    def first(i, watch):
        return HH.build(pkg, "c5000g")  # (kept to the end: host_threads.py, part C)

    def act(i, ctx, action, out):
        _churn, cloud, row = action
        ix = HH.build(pkg, cloud)
        try:
            got = HH.run(pkg, ix, cloud, row)
        finally:
            ix.close()
        for message in HT.differing(got, base[(cloud, row)]):
            out.failed("C", row, cloud, "thread %d" % i, message)

    def last(i, ctx):
        ctx.close()
    _conclude("C", *_threads(pkg, "C", HT.plan_c(), act, first, last))
