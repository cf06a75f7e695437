"""Every device-pointer entry point on a held stream (tests/stream_order.py): the promises of include/pcpx.h about streams that no
other test can see, because every other test drains the device around its calls.

Each row of tests/exact_buffers_cases.py runs twice on a handle built on one non-blocking stream S: plainly, on torch.full buffers
with the device drained around the call -- the form test_gpu_exact_buffers.py runs and the rest of the suite pins to its models;
it is also the warm-up, in which scratch may grow -- and then with S held by a timed kernel, the inputs delivered in stream order
behind it and every array taken back in stream order behind the call.

  a. ordered inputs and outputs: the held run's outputs are the plain run's, bit for bit, the caller's elements included.  A
     kernel that ran early, on another stream or before its inputs, read 0xA5; an output written late was snapshot too early;
  b. no late writes: once the device is drained every output still holds the 0x3C, and every input the 0xA5, that the stream put
     there behind the call;
  c. no hidden wait: a row that stream_order.WAITS classifies ENQUEUES returned while S was still held.  A row whose header
     documents a wait is held all the same, for a and b.

Nothing is compared with a tolerance and no shape is new: the table's clouds c70, c1300 and c5000g."""
import time

import pytest

import exact_buffers_cases as XC
import handle_history_cases as HH
import stream_order as SO

pytestmark = pytest.mark.gpu


def _torch():
    return pytest.importorskip("torch")


_state = {}
_handles = {}


def _line():
    """the session's stream and its delay: one calibration"""
    if "line" not in _state:
        t = _torch()
        device = t.device("cuda", 0)
        per_ms = SO.calibrate(t, t.cuda.Stream(device=device))
        stream = SO.independent_stream(t, device, per_ms)  # (not on the default stream's hardware queue)
        _state["per_ms"] = per_ms
        _state["line"] = SO.HeldLine(t, stream, per_ms * SO.DELAY_MS * 1.1)  # (a tenth more: DELAY_MS is the least it lasts)
    return _state["line"]


def _handle(pkg, cloud):
    if cloud not in _handles:
        _handles[cloud] = pkg.Index.from_device(HH.on_device(cloud).data_ptr(), HH.SIZES[cloud], stream=_line().handle,
                                                voxel_grid=HH.GRID if HH.gridded(cloud) else None)
        assert _handles[cloud].size() == int(HH.inputs(cloud)["inside"].sum())
    return _handles[cloud]


def test_the_stream_does_not_order_against_the_default_stream_and_the_delay_lasts():
    t = _torch()
    line = _line()
    stream = line.stream
    stream.synchronize()
    t0 = time.perf_counter()
    with line.on():
        line.hold()
    queued_ms = 1e3 * (time.perf_counter() - t0)
    marker = t.full((16,), 1, dtype=t.int32, device=line.device)  # (on the legacy default stream)
    t.cuda.current_stream().synchronize()
    assert not line.released(), "the default stream waited for the held stream: it is a blocking stream"
    stream.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)  # (host time: what a call that waits for the stream would see)
    assert line.released() and int(marker.sum()) == 16
    print("delay %.1f ms for %d ticks, %.0f ticks per ms, enqueued in %.3f ms" % (ms, line.ticks, _state["per_ms"], queued_ms))
    assert queued_ms < SO.DELAY_MS / 10, queued_ms
    assert SO.DELAY_MS <= ms <= 5 * SO.DELAY_MS, (ms, line.ticks)


CASES = [(row, cloud) for row in XC.ROWS for cloud in XC.clouds_of(row)]


@pytest.mark.parametrize("row,cloud", CASES, ids=["%s-%s" % c for c in CASES])
def test_a_row_on_a_held_stream(pkg, row, cloud):
    t = _torch()
    line = _line()
    ix = None if XC.ROWS[row].family == "free" else _handle(pkg, cloud)
    try:
        plain, _owned = XC.run(pkg, ix, cloud, row)
        t.cuda.synchronize()
        got, late, held = SO.run_held(pkg, ix, cloud, row, line)
    except AssertionError:
        raise
    except Exception as e:  # a HIP error: nothing more is started on a device that may have faulted
        pytest.exit("%s-%s: %s: %s" % (row, cloud, type(e).__name__, e), returncode=3)
    assert held.returned_before_release is not None, "the row made no call between a ready() and what follows it"
    print("%s-%s: the call returned after %.3f ms, the stream %s" % (row, cloud, 1e3 * held.call_seconds,
                                                                    "still held" if held.returned_before_release else "released"))
    found = ["(a) " + m for m in SO.differing_bits(got, plain)] + ["(b) " + m for m in late]
    if SO.WAITS[row] == SO.ENQUEUES and not held.returned_before_release:
        found.append("(c) the call waited for its stream: it returned after %.1f ms with the stream released, and %s promises that it only enqueues"
                     % (1e3 * held.call_seconds, ", ".join(XC.ROWS[row].symbols)))
    assert not found, (row, cloud, found)


def test_z_close_the_module_handles():
    t = _torch()
    for ix in _handles.values():
        ix.close()
    _handles.clear()
    t.cuda.synchronize()
