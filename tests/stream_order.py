"""Every device-pointer entry point on a stream that is HELD while the call is made: the run of tests/test_gpu_stream_order.py.  A
helper module, no conftest; its bookkeeping works on CPU tensors as on GPU ones (tests/test_stream_order_cpu.py).

Every other GPU test drains the device before a call and before it looks at an output, so a kernel on the wrong stream, a side
stream without an event join or a host wait inside a call that promises none all give the same bits.  Here a row of
tests/exact_buffers_cases.py runs on one non-blocking stream S (the legacy default stream does not order against it) that a timed
spin kernel holds for DELAY_MS, and its arrays exist only in stream order:

    up(data)      stages the data in a second device array, drains once, and returns a buffer full of the byte 0xA5 -- as an
                  index out of every range, as a float about -2.9e-16 (the over-read argument of tests/exact_buffers.py);
    first ready   enqueues on S, without a wait: the delay, an event `released`, the outputs' fill once more (what ran early and
                  wrote is overwritten) and copies of the staged data into the inputs: no array exists until the stream gets there;
    the call
    drain(), or   does not wait: it notes whether `released` has happened.  False: the call returned while the stream was still
    the ready()   held, so it waited for nothing on it
    after a call
    first down()  enqueues on S a snapshot of every buffer, then 0x3C into every output and 0xA5 into every input -- the caller owns
                  its arrays again once its stream has passed the call -- waits for S alone and answers from the snapshots;
    finish()      drains the device: every output still holds 0x3C and every input 0xA5, or something wrote late.

S is chosen by `independent_stream`: no order against the default stream is not yet concurrency with it, because a process's
streams share a few hardware queues, and S must not be the one that shares the default stream's.

A row that needs a host value between two calls is held for its first call only: a later ready() puts the snapshots back, delivers
what is new and waits for S.  A call that waits on the held stream only takes DELAY_MS longer: nothing here can hang.

WAITS classifies every row: ENQUEUES (the general rule of include/pcpx.h: a *_dev entry point "enqueues work on that stream and
returns without synchronising"), or the header and the phrase of it that documents the wait.

The delay is a condition, not a tolerance: a call that only enqueues must return well within it.  Measured on an MI355X with the
stream idle, on the library of the commit before this module: the host time from the first ready() to the note behind the row's
call or calls, warm (after the plain run), three times, the largest over the row's clouds -- MEASURED below, in ms.  Of the
ENQUEUES rows the largest are

    extract_planes 0.337 (max_planes rounds), icp_point 0.171 and icp_plane 0.127 (four iterations), voxel_grid 0.100,
    plane_ransac 0.074, ransac_rigid 0.061, nearest_posed 0.056, segment_curvature 0.053; a kNN call 0.006 to 0.045,
    bounding_box 0.021 with the wait it then still had (on an idle stream a wait costs nothing: why no timing shows one)

and the rows that document a wait took 0.08 (lists) to 0.96 ms (reconstruct).  Twenty times the largest is 6.7 ms, so the floor of
the rule, 50 ms, decides; DELAY_MS is twice that, 100 ms, which keeps a case near 0.13 s and the 129 of them under 20 s.
torch.cuda._sleep spins for a number of ticks of the device's cycle counter; `calibrate` times 20 000 000 of them (8.4 ms) with a
pair of events, once per session: 2.39 million ticks per ms on the MI355X.  The delay is sized a tenth longer than DELAY_MS and
test_gpu_stream_order.py asserts, by the host's clock, that it lasts at least DELAY_MS (109.4 ms when measured)."""
import contextlib
import time

import numpy as np

import exact_buffers as EB
import exact_buffers_cases as XC
import handle_history_cases as HH

INPUT_BYTE = EB.GUARD_BYTE  # 0xA5: what an input holds before the stream delivers it and after the stream has passed the call
AFTER_BYTE = 0x3C           # what an output holds after the stream has passed the call
DELAY_MS = 100.0
ENQUEUES = "enqueues"

# host ms of the warm call on an idle stream, the commit before this module (the docstring): row -> the largest over its clouds
MEASURED = {
    "knn_k8": 0.043, "knn_k15": 0.008, "knn_k32": 0.009, "knn_k40": 0.017, "knn_k15_pitch16": 0.007,
    "knn_k15_pitch16_slice": 0.008, "knn_k12_pitch16": 0.006, "knn_k12_pitch16_slice": 0.006, "knn_k3_pitch8": 0.006,
    "knn_k3_pitch8_slice": 0.007, "knn_k8_slice": 0.007, "knn_k32_slice": 0.006, "knn_batch_k8": 0.045, "knn_batch_k32": 0.045,
    "knn_curve_k8": 0.019, "knn_curve_k15": 0.018, "normals_k15": 0.006, "normals_k15_pitch16": 0.006,
    "normals_k12_pitch16_slice": 0.006, "neighbourhoods_k15": 0.006, "group_costs": 0.008, "propagate": 0.649, "sdf": 0.114,
    "reconstruct": 0.957, "count": 0.010, "count_slice": 0.009, "lists": 0.082, "moments": 0.011, "moments_slice": 0.008,
    "features": 0.011, "features_slice": 0.008, "mls": 0.022, "mls_slice": 0.013, "cluster_m5": 0.043,
    "cluster_m1_compact": 0.045, "segment": 0.051, "segment_curvature": 0.053, "subsample": 0.315, "local_maxima": 0.023,
    "iss": 0.032, "fpfh_all": 0.025, "fpfh_subset": 0.042, "nearest_posed": 0.056, "icp_point": 0.171, "icp_plane": 0.127,
    "surface_nets": 0.112, "surface_nets_timed": 0.144, "surface_nets_hint": 0.214, "surface_nets_hint_timed": 0.247,
    "bilateral_points": 0.311, "bilateral_normals": 0.345, "wlop": 0.580, "hierarchy": 0.917, "match_nearest": 0.024,
    "match_correspondences": 0.046, "ransac_rigid": 0.061, "rigid_fit": 0.037, "plane_ransac": 0.074, "plane_fit": 0.038,
    "extract_planes": 0.337, "voxel_grid": 0.100, "bounding_box": 0.021, "builds": 0.540,
}

_NETS = ("pcpx.h", "Synchronises `stream`")
_BILATERAL = ("pcpx.h", "return after the work has completed")
WAITS = {row: ENQUEUES for row in XC.ROWS}
WAITS.update({
    "propagate": ("pcpx.h", "synchronises `stream` once per 8 BFS levels"),
    "sdf": ("pcpx.h", "Enqueued on the handle's stream, which it synchronises"),
    "reconstruct": ("pcpx.h", "waits for the handle's stream more than once"),
    "lists": ("pcpx.h", "the call waits once, for the total"),
    "subsample": ("pcpx_subsample.h", "SYNCHRONISES the handle's stream between rounds"),
    "surface_nets": _NETS, "surface_nets_timed": _NETS, "surface_nets_hint": _NETS, "surface_nets_hint_timed": _NETS,
    "bilateral_points": _BILATERAL, "bilateral_normals": _BILATERAL,
    "wlop": ("pcpx.h", "pcpx_wlop_dev takes device arrays, runs on `stream` (NULL = the legacy default stream) and returns after the work has completed"),
    "hierarchy": ("pcpx.h", "enqueued on `stream`, which it synchronises"),
    "builds": ("pcpx.h", "wait for `stream` (a rebuild: the handle's) once, at the end of the build"),
})
PROMISES = ("no synchronisation", "never synchronise", "fully enqueued")  # a header that says one of these promises ENQUEUES


def normalised(text):
    return " ".join(text.replace("*", " ").replace("\\", " ").split())


# ---- the stream -------------------------------------------------------------------------------------------------------------------------
class HostLine:
    """the stand-in for a stream on CPU tensors: everything happens at once, nothing is ever held"""
    device, handle = "cpu", None

    def on(self):
        return contextlib.nullcontext()

    def hold(self):
        pass

    def released(self):
        return False

    def wait(self):
        pass

    def drain_device(self):
        pass


class HeldLine:
    """one non-blocking stream and the delay that holds it (ticks = 0: no delay, the stream is idle when the call is made)"""

    def __init__(self, torch, stream, ticks):
        self.torch, self.stream, self.ticks = torch, stream, int(ticks)
        self.device, self.handle, self.event = torch.device("cuda", 0), stream.cuda_stream, None

    def on(self):
        return self.torch.cuda.stream(self.stream)

    def hold(self):
        """(inside on()) the delay and the event behind it"""
        if self.ticks:
            self.torch.cuda._sleep(self.ticks)
        self.event = self.torch.cuda.Event()
        self.event.record(self.stream)

    def released(self):
        return bool(self.event.query())

    def wait(self):
        self.stream.synchronize()

    def drain_device(self):
        self.torch.cuda.synchronize()


def calibrate(torch, stream, ticks=2000000):
    """ticks of torch.cuda._sleep per millisecond on `stream`, by a pair of events around a delay of at least 5 ms: the largest of
    three readings (a delay sized by it lasts at least as long as asked for)"""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)  # (the kernel's code object is loaded)
        stream.synchronize()
        rates = []
        while len(rates) < 3:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            torch.cuda._sleep(ticks)
            e1.record(stream)
            stream.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0 or ticks >= 1 << 40:
                rates.append(ticks / ms)
            else:
                ticks *= 10
        return max(rates)


def independent_stream(torch, device, per_ms, tries=8, probe_ms=5.0):
    """a torch stream on whose delay work of the legacy default stream does not wait.  Every torch stream is non-blocking (no ORDER
    against the default stream), but the runtime maps a process's streams onto a few hardware queues in turn (four here: every
    fourth stream a process makes), and a kernel of the default stream that shares the held stream's queue starts behind the delay
    -- measured: its synchronisation then takes the whole delay, 0.05 ms otherwise.  Which stream that is depends on how many the
    process has made before, so each candidate is probed with a short delay; on such a stream work that slipped onto the default
    stream runs at once, reads 0xA5 and is seen.  The last candidate comes back if none is free (the GPU test then says so)."""
    for _ in range(tries):
        stream = torch.cuda.Stream(device=device)
        line = HeldLine(torch, stream, per_ms * probe_ms)
        stream.synchronize()
        with line.on():
            line.hold()
        torch.full((16,), 1, dtype=torch.int32, device=device)  # (on the legacy default stream)
        torch.cuda.current_stream(device).synchronize()
        free = not line.released()
        stream.synchronize()
        if free:
            break
    return stream


# ---- the buffers ------------------------------------------------------------------------------------------------------------------------
class _Buffer:
    def __init__(self, name, tensor, role, staged=None):
        self.name, self.tensor, self.role, self.staged, self.snapshot = name, tensor, role, staged, None


def _torch():
    import torch
    return torch


def _bytes(t):
    return t.view(_torch().uint8)


class Held(XC.Buffers):
    """exact_buffers_cases.Buffers on a held stream (the module's docstring)"""

    def __init__(self, pkg, ix, cloud, line):
        super().__init__(pkg, ix, cloud)
        self.line, self.stream = line, line.handle
        self.buffers, self.state = [], "fresh"  # fresh -> held (the first call is being made) -> open <-> closed
        self.returned_before_release = None     # True: the first call returned while the stream was still held
        self.call_seconds = None                # host seconds between the first ready() and the note that follows the call
        self._t0 = None

    # the arrays
    def out(self, length, kind, name=None):
        t = _torch()
        dtype = {"u32": t.int32, "u64": t.int64, "u8": t.uint8, "f32": t.float32, "f64": t.float64}[kind]
        with self.line.on():
            d = t.full((max(int(length), 1),), HH.FILL, dtype=dtype, device=self.line.device)
        self.buffers.append(_Buffer(name or self._name("output " + kind), d, "output"))
        return d

    def up(self, a, name=None):
        t = _torch()
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
        staged = t.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype)).to(self.line.device)
        with self.line.on():
            d = t.full((staged.numel() * staged.element_size(),), INPUT_BYTE, dtype=t.uint8, device=self.line.device).view(staged.dtype)
        self.line.drain_device()
        self.buffers.append(_Buffer(name or self._name("input " + EB.kind_of(a)), d, "input", staged))
        return d

    def _deliver(self):
        for b in self.buffers:
            if b.snapshot is not None:  # (a later phase of the row: every array as the stream left it)
                b.tensor.copy_(b.snapshot)
                b.snapshot = None
            elif b.staged is not None:
                b.tensor.copy_(b.staged)
            b.staged = None

    def _note(self):
        self.call_seconds = time.perf_counter() - self._t0
        self.returned_before_release = not self.line.released()
        self.state = "open"

    # the hooks of a row
    def ready(self):
        if self.state == "fresh":
            with self.line.on():
                self.line.hold()
                for b in self.buffers:
                    if b.role == "output":
                        b.tensor.fill_(HH.FILL)  # (once more, behind the delay: what a kernel wrote early is gone)
                self._deliver()
            if not getattr(self.line, "ticks", 1):
                self.line.wait()  # (the measuring form: an idle stream)
            self.state, self._t0 = "held", time.perf_counter()
        elif self.state == "held":
            self._note()
        else:
            with self.line.on():
                self._deliver()
            self.line.wait()
            self.state = "open"

    def drain(self):
        if self.state == "held":
            self._note()
        else:
            self.line.wait()

    def _close(self):
        if self.state == "held":
            self._note()
        with self.line.on():
            for b in self.buffers:
                b.snapshot = b.tensor.clone()
            for b in self.buffers:
                if b.role == "output":
                    _bytes(b.tensor).fill_(AFTER_BYTE)
            for b in self.buffers:
                if b.role == "input":
                    _bytes(b.tensor).fill_(INPUT_BYTE)
        self.line.wait()
        self.state = "closed"

    def down(self, d, length=None, width=1):
        if self.state != "closed":
            self._close()
        b = [b for b in self.buffers if b.tensor is d][0]
        return super().down(b.snapshot, length, width)

    def finish(self):
        """after the row: the device drained, and the late writes as a list of messages"""
        if self.state != "closed":
            self._close()
        self.line.drain_device()
        return self.late_writes()

    def late_writes(self):
        t = _torch()
        found = []
        for b in self.buffers:
            want = AFTER_BYTE if b.role == "output" else INPUT_BYTE
            bad = _bytes(b.tensor) != want
            if bool(bad.any()):
                at = int(t.nonzero(bad)[0, 0])
                found.append("a write after the stream had passed the call: byte %d of %r (%s, %d bytes) is 0x%02X, not 0x%02X; %d byte(s) changed in all"
                             % (at, b.name, b.role, bad.numel(), int(_bytes(b.tensor)[at]), want, int(bad.sum())))
        return found


def run_held(pkg, ix, cloud, row, line):
    """(the row's outputs on the held stream as contiguous host arrays, the late writes, the Held)"""
    c = Held(pkg, ix, cloud, line)
    got = {k: np.ascontiguousarray(v) for k, v in XC.ROWS[row].fn(c).items()}
    return got, c.finish(), c


def differing_bits(got, plain):
    """(a): the keys, types, shapes and bits of a held run against the plain run's, as a list of messages"""
    if sorted(got) != sorted(plain):
        return ["outputs %s, the plain run's %s" % (sorted(got), sorted(plain))]
    found = []
    for key, a in got.items():
        p = plain[key]
        if a.dtype != p.dtype or a.shape != p.shape:
            found.append("%s: %s %s, the plain run's %s %s" % (key, a.dtype, a.shape, p.dtype, p.shape))
            continue
        bad = np.nonzero((HH.bits(a) != HH.bits(p)).reshape(-1))[0]
        if len(bad):
            found.append("%s: %d element(s) differ from the plain run's, the first at %s: %s, there %s"
                         % (key, len(bad), bad[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), p.reshape(-1)[bad[:4]].tolist()))
    return found
