"""Every entry point from several host threads at once: the plans, the threads and the counting of tests/test_gpu_host_threads.py.
A helper module, no conftest; the plans are plain data and are proved on the CPU (tests/test_host_threads_cpu.py).

include/pcpx.h (Conventions, "Threads") promises that any entry point may be called from any thread at any time: calls on one
handle run one at a time, the entry points that stage through a device's shared pool run one at a time per device, handles are
independent of one another, and the error text and the current device are the calling thread's.  Every other test calls the
library from one thread with the device drained around the call, so none of the state that those promises rest on -- a handle's
mutex, the device's pool and its lock, the list of leased blocks, the cache of index blocks, the pooled streams, the upload ring,
the hint mesher's search-order table, the thread's error text, the device scope -- is ever contended.  Here T = 8 Python threads
of the one test process call the library side by side (ctypes releases the GIL for the duration of a call):

    part A  every thread builds its own handles on its own non-blocking stream and runs its share of exact_buffers_cases.ROWS on
            arrays of that stream (Threaded), waiting for that stream only: the rows without a handle queue on eight streams
    part B  one handle per home cloud of handle_history_cases, shared by all threads, runs handle_history_cases.ROWS through
            handle_history_cases.run as it is; one thread rebuilds the handles to their own clouds in between
    part C  every thread six times: a handle from host memory (c33000, above the upload ring's threshold, and c5000g in turn), one
            row, close -- what one thread's handle gives back becomes another thread's tree.  Every thread also keeps one more
            handle from its first step to its last: sixteen private streams exist, so when the last eight handles are closed, side by
            side, the pool of idle streams is full and the branch that destroys a stream runs
    part D  inside A and B: between its rows a thread makes a call that its argument check refuses and finds its own radius in its
            own error text, before and after its next successful call; with two devices or more half of B's threads have device 1
            current and find it current after every call

A row's expected result is never threaded code: A compares with exact_buffers_cases.run on the main thread, B and C with
handle_history_cases.fresh, both made before the first thread starts, and every comparison is of bits, the caller's elements
included.  The threads walk a plan in steps with a barrier before each, so the plan decides what runs side by side; every row of a
part is dealt to exactly two different threads at different steps.

Two conditions keep this honest.  Overlap: while the threads run, every function of the loaded library is behind a thin wrapper
(Watch) that counts the calls that began while a call of ANOTHER thread was inside the library; a part asserts that the count is
positive.  On one shared handle such a call is one that waited at the handle's mutex: the count is the same.  No wait without an
end: the threads are daemon threads, every barrier and the join have a limit (`limit_for`), and a thread that has not come back or
a call that raised anything but an assertion ends the session (the GPU test; nothing more is started on the device)."""
import ctypes as C
import math
import threading
import time

import numpy as np

import exact_buffers_cases as XC
import handle_history_cases as HH
import stream_order as SO

T = 8
FAMILIES = ("knn", "any", "free")
FAIL_EVERY = 3          # thread t makes its refused call after its row of the steps s with (s + t) % FAIL_EVERY == 0
REBUILDER = 0           # the thread of part B that rebuilds the shared handles
CHURN = 6               # handles per thread in part C
CHURN_CASES = (("c33000", "knn_dev_k8"), ("c5000g", "count_self_dev"))
LIMIT_FACTOR, LIMIT_FLOOR = 20.0, 30.0
NOT_COUNTED = ("pcpx_last_error", "pcpx_abi_version")  # (they enter nothing)


def limit_for(baseline_seconds):
    """seconds a barrier or the join may take: a cap against a deadlock, not a performance claim"""
    return max(LIMIT_FLOOR, LIMIT_FACTOR * float(baseline_seconds))


# ---- the plans ------------------------------------------------------------------------------------------------------------------------
# A plan is a list of steps; a step has one list of actions per thread; an action is ("row", row), ("fail",), ("rebuild", cloud)
# or ("churn", cloud, row).
def family_a(row):
    return XC.ROWS[row].family


def family_b(row):
    return HH.ROWS[row][0]


def _deal(order, threads):
    """steps of `threads` entries (None: idle) from a list of items: entry t of step s is item threads * s + t"""
    order = list(order) + [None] * (-len(order) % threads)
    return [order[i:i + threads] for i in range(0, len(order), threads)]


def _dealt_twice(items, family_of, threads=T):
    """every item twice: once in table order -- the table lists a family together, so these steps put rows of one family side by
    side -- and once in a strided order that mixes the families; the first (stride, start) under which every item falls to two
    different threads at different steps and every pair of families shares a step"""
    items = list(items)
    n = len(items)
    want = {tuple(sorted((a, b))) for a in FAMILIES for b in FAMILIES}
    for stride in range(2, n):
        if math.gcd(stride, n) != 1:
            continue
        for start in range(n):
            second = [items[(start + i * stride) % n] for i in range(n)]
            steps = _deal(items + second, threads)
            at = {}
            for s, step in enumerate(steps):
                for t, item in enumerate(step):
                    if item is not None:
                        at.setdefault(item, []).append((s, t))
            if any(len(v) != 2 or v[0][0] == v[1][0] or v[0][1] == v[1][1] for v in at.values()):
                continue
            pairs = set()
            for step in steps:
                fams = [family_of(i) for i in step if i is not None]
                pairs |= {tuple(sorted((a, b))) for i, a in enumerate(fams) for b in fams[i + 1:]}
            if want <= pairs:
                return steps
    raise AssertionError("no deal of %d items over %d threads meets the plan's conditions" % (n, threads))


def _with_fails(steps):
    out = []
    for s, step in enumerate(steps):
        out.append([([("row", item)] if item is not None else []) + ([("fail",)] if (s + t) % FAIL_EVERY == 0 else []) for t, item in enumerate(step)])
    return out


def plan_a():
    """part A: exact_buffers_cases.ROWS, a row on every cloud of clouds_of(row)"""
    return _with_fails(_dealt_twice(XC.ROWS, family_a))


def plan_b():
    """part B: handle_history_cases.ROWS on their home clouds; thread REBUILDER rebuilds a shared handle before its row of every
    step but the first, the two home clouds in turn"""
    steps = _with_fails(_dealt_twice(HH.ROWS, family_b))
    homes = shared_clouds()
    for s, step in enumerate(steps):
        if s > 0:
            step[REBUILDER].insert(0, ("rebuild", homes[s % len(homes)]))
    return steps


def plan_c():
    """part C: CHURN steps; thread t's i-th handle is on CHURN_CASES[(i + t) % 2], so both clouds are built side by side"""
    return [[[("churn",) + CHURN_CASES[(i + t) % len(CHURN_CASES)]] for t in range(T)] for i in range(CHURN)]


def shared_clouds():
    """the clouds of part B's shared handles: the home clouds of the families that take a handle"""
    return tuple(HH.HOME[f] for f in FAMILIES if f != "free")


def home_of(row):
    return HH.HOME[family_b(row)]


def rows_of(plan):
    """row -> [(step, thread)] over a plan's "row" actions"""
    at = {}
    for s, step in enumerate(plan):
        for t, actions in enumerate(step):
            for a in actions:
                if a[0] == "row":
                    at.setdefault(a[1], []).append((s, t))
    return at


def family_pairs(plan, family_of):
    """the pairs of families that some step has two threads in at once"""
    pairs = set()
    for step in plan:
        fams = [family_of(a[1]) for actions in step for a in actions if a[0] == "row"]
        pairs |= {tuple(sorted((a, b))) for i, a in enumerate(fams) for b in fams[i + 1:]}
    return pairs


# ---- the counting -----------------------------------------------------------------------------------------------------------------------
class _Counted:
    """a function of the loaded library behind the count (its other attributes are the function's)"""

    def __init__(self, watch, name, fn):
        self._watch, self._name, self._fn = watch, name, fn

    def __getattr__(self, key):
        return getattr(self._fn, key)

    def __call__(self, *args):
        w, me = self._watch, threading.get_ident()
        with w.lock:
            mine = w.inside.get(me, 0)
            w.calls += 1
            if w.total_inside > mine:
                w.overlapped += 1
            w.inside[me] = mine + 1
            w.total_inside += 1
        try:
            return self._fn(*args)
        finally:
            with w.lock:
                w.inside[me] -= 1
                w.total_inside -= 1
            want = w.expect.get(me)
            if want is not None and w.current_device is not None:
                now = w.current_device()
                if now != want:
                    w.moved.append("%s left device %d current on a thread whose current device was %d" % (self._name, now, want))


class Watch:
    """While installed, every named function of `lib` (the one ctypes.CDLL that the package calls through) counts its calls:
    `calls` in all, `overlapped` those that began while another thread was inside the library.  expect[thread ident] = the device
    that must be current on that thread after every call (`current_device` reads it); `moved` lists the calls after which it
    was not."""

    def __init__(self, lib, names, current_device=None):
        self.lib, self.names, self.current_device = lib, [n for n in names if n not in NOT_COUNTED], current_device
        self.lock = threading.Lock()
        self.inside, self.total_inside, self.calls, self.overlapped = {}, 0, 0, 0
        self.expect, self.moved, self._saved = {}, [], {}

    def __enter__(self):
        for name in self.names:
            self._saved[name] = getattr(self.lib, name)
            setattr(self.lib, name, _Counted(self, name, self._saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.lib, name, fn)
        self._saved = {}
        return False


# ---- the threads ------------------------------------------------------------------------------------------------------------------------
class Outcome:
    def __init__(self):
        self.lock = threading.Lock()
        self.failures = []  # what a comparison or an assertion found: the test fails
        self.fatal = []     # anything else a call raised (a HIP error): the session ends
        self.hung = []      # threads that had not come back by the limit: the session ends
        self.seconds = 0.0

    def failed(self, *what):
        with self.lock:
            self.failures.append(what)


def run_plan(plan, act, limit, first=None, last=None, threads=T):
    """Walks `plan` with `threads` daemon threads: thread t calls first(t) -> its context, then behind a barrier per step
    act(t, context, action, outcome) for its actions of the step, and behind a last barrier last(t, context).  A comparison that
    differs is reported through outcome.failed and the plan goes on; an assertion raised ends the plan for every thread (the
    barrier is aborted), anything else raised is fatal.  No barrier and no join waits longer than `limit` seconds."""
    out = Outcome()
    barrier = threading.Barrier(threads, timeout=limit)

    def walk(t):
        try:
            barrier.wait()
            ctx = first(t) if first else None
            for step in plan:
                barrier.wait()
                for action in step[t]:
                    act(t, ctx, action, out)
            barrier.wait()
            if last:
                last(t, ctx)
        except threading.BrokenBarrierError:
            pass  # (another thread has said why, or the limit has passed: the join says so)
        except AssertionError as e:
            out.failed("thread %d" % t, "AssertionError", str(e))
            barrier.abort()
        except BaseException as e:
            with out.lock:
                out.fatal.append("thread %d: %s: %s" % (t, type(e).__name__, e))
            barrier.abort()

    workers = [threading.Thread(target=walk, args=(t,), name="host-thread-%d" % t, daemon=True) for t in range(threads)]
    t0 = time.perf_counter()
    for w in workers:
        w.start()
    for w in workers:
        w.join(max(0.0, t0 + limit - time.perf_counter()))
    out.hung = [w.name for w in workers if w.is_alive()]
    if barrier.broken and not out.hung and not out.fatal and not out.failures:
        out.hung = ["a barrier waited longer than %.0f s" % limit]
    out.seconds = time.perf_counter() - t0
    return out


# ---- part A: arrays of the thread's own stream ------------------------------------------------------------------------------------------
class Threaded(XC.Buffers):
    """exact_buffers_cases.Buffers on one thread's torch stream: the arrays are made and filled in that stream's order, ready()
    waits for that stream only, and `stream` -- what a row passes to a call that takes one -- is its handle"""

    def __init__(self, pkg, ix, cloud, torch_stream):
        super().__init__(pkg, ix, cloud)
        self.on, self.stream = torch_stream, torch_stream.cuda_stream

    def _device(self):
        return self.torch().device("cuda", 0)

    def out(self, length, kind, name=None):
        t = self.torch()
        dtype = {"u32": t.int32, "u64": t.int64, "u8": t.uint8, "f32": t.float32, "f64": t.float64}[kind]
        with t.cuda.stream(self.on):
            return t.full((max(int(length), 1),), HH.FILL, dtype=dtype, device=self._device())

    def up(self, a, name=None):
        t = self.torch()
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
        with t.cuda.stream(self.on):
            return t.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype)).to(self._device())

    def ready(self):
        self.on.synchronize()

    def down(self, d, length=None, width=1):
        with self.torch().cuda.stream(self.on):
            return super().down(d, length, width)


def run_threaded(pkg, ix, cloud, row, torch_stream):
    """the row's outputs through a Threaded, as contiguous host arrays"""
    return {k: np.ascontiguousarray(v) for k, v in XC.ROWS[row].fn(Threaded(pkg, ix, cloud, torch_stream)).items()}


# ---- part D: the refused call -------------------------------------------------------------------------------------------------------------
def radius_of(t):
    return -(1.0 + t)


def refused_call(lib, capi, ix, t, d_counts):
    """The counting form of the sphere walk with radius -(1 + t), which check_radius refuses before anything is launched (the plain
    pcpx_range_count_* forms take any radius: they have no such check), then pcpx_index_size, which succeeds.  Returns what is
    wrong as a list of messages: the status, the thread's error text after the refusal, the text after the success."""
    found = []
    st = lib.pcpx_range_neighbourhoods_self_dev(ix._h, radius_of(t), 0, capi.UINT64_MAX, None, None, None, C.c_void_p(d_counts))
    text = (lib.pcpx_last_error() or b"").decode("utf-8", "replace")
    mine = "(got %g)" % radius_of(t)
    if st != capi.PCPX_ERR_INVALID:
        found.append("radius %g: status %d, not PCPX_ERR_INVALID" % (radius_of(t), st))
    if not text.endswith(mine):
        found.append("thread %d: the error text after its refused call is %r, which does not end in %r" % (t, text, mine))
    n = C.c_uint64(0)
    st = lib.pcpx_index_size(ix._h, C.byref(n))
    after = (lib.pcpx_last_error() or b"").decode("utf-8", "replace")
    if st != capi.PCPX_OK:
        found.append("pcpx_index_size: status %d (%s)" % (st, after))
    if after != text or not after.endswith(mine):
        found.append("thread %d: the error text after its next successful call is %r, it was %r" % (t, after, text))
    return found


def differing(got, want):
    """handle_history_cases.same_bits as a list of messages"""
    try:
        HH.same_bits(got, want, "bits")
    except AssertionError as e:
        return [str(e)]
    return []


differing_bits = SO.differing_bits
