"""The plans of tests/host_threads.py, proved without a GPU: what runs side by side in tests/test_gpu_host_threads.py is decided here,
not by the scheduler.  Also the bookkeeping that the GPU test relies on -- the overlap count and the limits of the threads -- on
plain Python callables."""
import threading

import exact_buffers_cases as XC
import handle_history_cases as HH
import host_threads as HT

ALL_PAIRS = {tuple(sorted((a, b))) for a in HT.FAMILIES for b in HT.FAMILIES}


def _check_deal(plan, rows, family_of):
    at = HT.rows_of(plan)
    assert sorted(at) == sorted(rows)  # every row, and no other
    for row, where in at.items():
        assert len(where) == 2, (row, where)
        (s0, t0), (s1, t1) = where
        assert s0 != s1 and t0 != t1, (row, where)  # two different threads, at different steps
    assert HT.family_pairs(plan, family_of) == ALL_PAIRS
    for step in plan:
        assert len(step) == HT.T
        for actions in step:
            assert sum(a[0] == "row" for a in actions) <= 1  # a thread runs one row per step


def _fails_of(plan):
    """thread -> the steps in which it makes its refused call, each behind the step's row"""
    out = {}
    for s, step in enumerate(plan):
        for t, actions in enumerate(step):
            if ("fail",) in actions:
                assert actions[-1] == ("fail",) and actions.count(("fail",)) == 1
                out.setdefault(t, []).append(s)
    return out


def test_part_a_deals_every_row_to_two_threads_and_every_pair_of_families_to_a_step():
    plan = HT.plan_a()
    _check_deal(plan, XC.ROWS, HT.family_a)
    assert {HT.family_a(r) for r in XC.ROWS} == set(HT.FAMILIES)
    for row in XC.ROWS:  # a thread has a handle on every cloud of the table, and a row asks for no other
        assert 0 < len(XC.clouds_of(row)) <= len(XC.CLOUDS) and set(XC.clouds_of(row)) <= set(XC.CLOUDS) <= set(HH.SIZES)
    fails = _fails_of(plan)
    assert sorted(fails) == list(range(HT.T)) and all(len(v) >= 2 for v in fails.values())  # every thread, between its rows
    assert len({HT.radius_of(t) for t in range(HT.T)}) == HT.T and all(HT.radius_of(t) < 0 for t in range(HT.T))
    assert len({"%g" % HT.radius_of(t) for t in range(HT.T)}) == HT.T  # (no thread's text ends like another's)


def test_part_b_deals_every_row_on_its_home_cloud_and_has_the_rebuilds():
    plan = HT.plan_b()
    _check_deal(plan, HH.ROWS, HT.family_b)
    assert HT.shared_clouds() == ("c5000", "c5000g")
    for row in HH.ROWS:
        assert HH.runs_on(row, HT.home_of(row)) and HT.home_of(row) in HH.SIZES
        assert HT.family_b(row) == "free" or HT.home_of(row) in HT.shared_clouds()
    fails = _fails_of(plan)
    assert sorted(fails) == list(range(HT.T)) and all(len(v) >= 2 for v in fails.values())
    rebuilds = [(s, t, a[1]) for s, step in enumerate(plan) for t, actions in enumerate(step) for a in actions if a[0] == "rebuild"]
    assert {t for _s, t, _c in rebuilds} == {HT.REBUILDER}  # one thread rebuilds ...
    assert {c for _s, _t, c in rebuilds} == set(HT.shared_clouds())  # ... every shared handle, to its own cloud ...
    for s, t, _c in rebuilds:  # ... between its rows, while the other threads run theirs
        assert 0 < s and any(a[0] == "row" for a in plan[s][t]) and any(a[0] == "row" for u in range(HT.T) if u != t for a in plan[s][u])


def test_part_c_builds_both_clouds_side_by_side_six_times_per_thread():
    plan = HT.plan_c()
    assert len(plan) == HT.CHURN == 6
    for step in plan:
        assert len(step) == HT.T and all(len(actions) == 1 and actions[0][0] == "churn" for actions in step)
        assert {actions[0][1] for actions in step} == {"c33000", "c5000g"}
    for t in range(HT.T):
        clouds = [step[t][0][1] for step in plan]
        assert all(a != b for a, b in zip(clouds, clouds[1:]))  # alternately
    for cloud, row in HT.CHURN_CASES:
        assert HH.runs_on(row, cloud)
    assert HH.SIZES["c33000"] * 12 > 64 << 10  # above the upload ring's threshold (pcpx_runtime.hip: upload_pageable)


def test_the_plans_are_the_same_every_time():
    assert HT.plan_a() == HT.plan_a() and HT.plan_b() == HT.plan_b() and HT.plan_c() == HT.plan_c()


def test_limits():
    assert HT.limit_for(0.0) == 30.0 and HT.limit_for(1.0) == 30.0 and HT.limit_for(2.5) == 50.0


class _Lib:
    """stands in for the loaded library: two functions, one of which two threads can be inside at once"""

    def __init__(self):
        self.gate = threading.Barrier(2, timeout=10)

    def pcpx_together(self):
        self.gate.wait()  # (returns only when both threads are inside)
        return 0

    def pcpx_alone(self):
        return 0

    def pcpx_last_error(self):
        return b""


def test_the_watch_counts_only_calls_that_began_with_another_thread_inside():
    lib = _Lib()
    plain = lib.pcpx_alone
    with HT.Watch(lib, ["pcpx_together", "pcpx_alone", "pcpx_last_error"]) as w:
        for _ in range(5):
            lib.pcpx_alone()
            lib.pcpx_last_error()
        assert (w.calls, w.overlapped) == (5, 0)  # one thread: nothing overlaps; pcpx_last_error is not counted
        threads = [threading.Thread(target=lib.pcpx_together, daemon=True) for _ in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(10)
        assert not any(th.is_alive() for th in threads)
        assert (w.calls, w.overlapped) == (7, 1)  # the second to enter found the first inside
        assert w.total_inside == 0
    assert lib.pcpx_alone == plain and not isinstance(lib.pcpx_together, HT._Counted)  # removed again


def test_the_watch_reports_a_current_device_that_a_call_changed():
    lib = _Lib()
    device = [1]

    def moves():
        device[0] = 0
        return 0
    lib.pcpx_moves = moves
    with HT.Watch(lib, ["pcpx_alone", "pcpx_moves"], current_device=lambda: device[0]) as w:
        w.expect[threading.get_ident()] = 1
        lib.pcpx_alone()
        assert w.moved == []
        lib.pcpx_moves()
        assert len(w.moved) == 1 and "pcpx_moves" in w.moved[0]


def test_run_plan_walks_the_steps_behind_barriers_and_ends_a_wait():
    plan = [[[("row", "s%d" % s)] for _t in range(HT.T)] for s in range(3)]
    seen, lock = [], threading.Lock()

    def act(t, ctx, action, out):
        with lock:
            seen.append((action[1], t, ctx))
        if action[1] == "s1" and t == 2:
            out.failed("thread 2", "differs")
    out = HT.run_plan(plan, act, 10.0, first=lambda t: 10 + t)
    assert not out.fatal and not out.hung and out.failures == [("thread 2", "differs")]
    assert [s for s, _t, _c in seen] == sorted(s for s, _t, _c in seen) and len(seen) == 3 * HT.T  # no thread ran ahead of a step
    assert all(c == 10 + t for _s, t, c in seen)

    def raises(t, ctx, action, out):
        if t == 1:
            raise RuntimeError("a HIP error")
    out = HT.run_plan(plan, raises, 10.0)
    assert len(out.fatal) == 1 and "RuntimeError" in out.fatal[0] and not out.hung

    def asserts(t, ctx, action, out):
        assert t != 4, "thread 4 found something"
    out = HT.run_plan(plan, asserts, 10.0)
    assert not out.fatal and not out.hung and len(out.failures) == 1 and "thread 4 found something" in out.failures[0][2]
