"""What tests/test_gpu_stream_order.py rests on, checked without a GPU: that stream_order.WAITS classifies exactly the rows of
tests/exact_buffers_cases.py, every wait by a phrase that its header really holds and every promise of the headers as ENQUEUES,
and the bookkeeping of stream_order.Held on CPU tensors."""
import os
import re

import numpy as np
import pytest

import exact_buffers_cases as XC
import handle_history_cases as HH
import stream_order as SO

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header(name):
    return open(os.path.join(INCLUDE, name)).read()


def _headers():
    return sorted(f for f in os.listdir(INCLUDE) if re.fullmatch(r"pcpx\w*\.h", f))


def _said_of(symbol):
    """(header, what it says of the entry point, normalised): the comment in front of its declaration, back to the declaration before
    it, and for the family headers (every one but pcpx.h, whose opening comment states the general rule) the header's opening comment"""
    for name in _headers():
        text = _header(name)
        m = re.search(r"^int %s\(" % re.escape(symbol), text, re.M)
        if not m:
            continue
        lines = []
        for line in reversed(text[:m.start()].split("\n")):
            if line.strip() and not line.startswith(("/*", " *")):
                break
            lines.insert(0, line)
        said = "\n".join(lines)
        if name != "pcpx.h":
            said = text[:text.find("*/")] + " " + said
        return name, SO.normalised(said)
    raise AssertionError("%s is declared in no header" % symbol)


# ---- the classification -------------------------------------------------------------------------------------------------------------------
def test_waits_has_exactly_the_rows_of_the_table():
    assert set(SO.WAITS) == set(XC.ROWS)
    for row, w in SO.WAITS.items():
        assert w == SO.ENQUEUES or (isinstance(w, tuple) and len(w) == 2 and w[0] in _headers() and len(w[1].split()) >= 2), (row, w)
    assert sum(w == SO.ENQUEUES for w in SO.WAITS.values()) >= 40 and sum(w != SO.ENQUEUES for w in SO.WAITS.values()) >= 14


@pytest.mark.parametrize("row", [r for r, w in SO.WAITS.items() if w != SO.ENQUEUES])
def test_a_documented_wait_is_in_the_header_it_names(row):
    header, phrase = SO.WAITS[row]
    assert SO.normalised(phrase) in SO.normalised(_header(header)), (row, header, phrase)
    # ... and in the header of one of the row's own entry points
    assert header in {_said_of(s)[0] for s in XC.ROWS[row].symbols}, (row, header)


def test_the_general_rule_is_still_what_the_header_states():
    text = SO.normalised(_header("pcpx.h"))
    assert "they enqueue work on that stream and return without synchronising" in text
    assert "A NULL stream is the legacy default stream" in text and "never a private one" in text


def test_a_row_whose_header_promises_no_wait_is_classified_enqueues():
    promised = []
    for row, r in XC.ROWS.items():
        for symbol in r.symbols:
            header, said = _said_of(symbol)
            hit = [p for p in SO.PROMISES if p in said.lower()]
            if hit:
                promised.append(row)
                assert SO.WAITS[row] == SO.ENQUEUES, (row, symbol, header, hit)
    # the families of the README's device pipeline are among them
    for row in ("match_nearest", "match_correspondences", "ransac_rigid", "rigid_fit", "plane_ransac", "plane_fit", "extract_planes", "voxel_grid",
                "icp_point", "icp_plane", "nearest_posed", "fpfh_all", "local_maxima", "bounding_box"):
        assert row in promised, row


def test_a_header_that_documents_a_wait_promises_none():
    """no entry point has it both ways: a comment that promises no wait and one that a WAITS phrase quotes"""
    for row, w in SO.WAITS.items():
        if w == SO.ENQUEUES:
            continue
        for symbol in XC.ROWS[row].symbols:
            header, said = _said_of(symbol)
            assert not [p for p in SO.PROMISES if p in said.lower()], (row, symbol, header)


# ---- the bookkeeping on CPU tensors -------------------------------------------------------------------------------------------------------
def _held():
    c = SO.Held(None, None, "c70", SO.HostLine())
    assert c.stream is None and c.state == "fresh"
    return c


def _raw(t):
    return t.view(torch.uint8).numpy()


def test_an_input_exists_only_after_the_first_ready_and_is_taken_back_at_the_first_down():
    c = _held()
    data = np.array([1.5, -0.0, np.nan, 3.0], np.float32)
    rows = np.array([3, 2 ** 32 - 1], np.uint32)
    d, r, o = c.up(data), c.up(rows, "rows"), c.out(5, "u64")
    assert (_raw(d) == SO.INPUT_BYTE).all() and (_raw(r) == SO.INPUT_BYTE).all() and d.dtype == torch.float32 and r.dtype == torch.int32
    assert (o.numpy() == HH.FILL).all() and o.dtype == torch.int64
    o[4] = 99  # (a kernel that ran before the stream got to the call)
    c.ready()
    assert int(o[4]) == HH.FILL, "the outputs are filled behind the delay as well"
    assert c.state == "held" and d.numpy().tobytes() == data.tobytes() and r.numpy().view(np.uint32).tolist() == rows.tolist()
    o[:3] = torch.tensor([10, 11, 12])  # (the call)
    d[1] = 9.0                            # (an array updated in place)
    c.drain()
    assert c.state == "open" and c.returned_before_release is True and c.call_seconds >= 0.0
    got = c.down(o, 4)
    assert c.state == "closed" and got.dtype == np.uint64 and got.tolist() == [10, 11, 12, HH.FILL]
    assert c.down(d, 4).tobytes() == np.array([1.5, 9.0, np.nan, 3.0], np.float32).tobytes()
    assert c.down(r).dtype == np.uint32
    # the stream has passed the call: the caller's arrays are the caller's again
    assert (_raw(o) == SO.AFTER_BYTE).all() and (_raw(d) == SO.INPUT_BYTE).all() and (_raw(r) == SO.INPUT_BYTE).all()
    assert c.finish() == []


def test_a_ready_after_a_call_notes_and_a_later_one_puts_the_arrays_back():
    """the rows that need a host value between two calls: held for the first call, every array as the stream left it for the second"""
    c = _held()
    d, count = c.up(np.arange(6, dtype=np.float32)), c.out(1, "u64")
    c.ready()
    count[0] = 4
    c.ready()
    assert c.state == "open" and c.returned_before_release is True
    assert int(c.down(count, 1)[0]) == 4 and (_raw(d) == SO.INPUT_BYTE).all() and (_raw(count) == SO.AFTER_BYTE).all()
    rows = c.out(4, "u32")
    c.ready()
    assert c.state == "open" and d.numpy().tolist() == [0, 1, 2, 3, 4, 5] and int(count[0]) == 4 and (rows.numpy() == HH.FILL).all()
    rows[:] = torch.tensor([5, 6, 7, 8], dtype=torch.int32)
    c.ready()
    assert c.down(rows, 4, 2).tolist() == [[5, 6], [7, 8]] and int(c.down(count, 1)[0]) == 4
    assert (_raw(rows) == SO.AFTER_BYTE).all() and (_raw(d) == SO.INPUT_BYTE).all()
    assert c.finish() == []


def test_a_row_without_a_down_is_closed_by_finish():
    c = _held()
    d = c.up(np.arange(3, dtype=np.uint32))
    c.ready()
    assert c.finish() == [] and c.returned_before_release is True and (_raw(d) == SO.INPUT_BYTE).all()


@pytest.mark.parametrize("role", ["output", "input"])
def test_a_byte_written_after_the_stream_has_passed_the_call_is_reported(role):
    c = _held()
    d, o = c.up(np.zeros(9, np.float32), "the cloud"), c.out(7, "u32", "the counts")
    c.ready()
    c.drain()
    c.down(o, 7)
    victim = o if role == "output" else d
    _raw(victim)[13] = 0x01  # (planted: a kernel on a side stream that finishes late)
    late = c.finish()
    assert len(late) == 1, late
    name = "'the counts'" if role == "output" else "'the cloud'"
    assert name in late[0] and "byte 13 of" in late[0] and "0x01" in late[0] and "1 byte(s) changed" in late[0], late


def test_differing_bits_sees_one_bit_and_the_sign_of_zero():
    plain = {"a": np.array([1.0, 0.0, 2.0], np.float32), "n": np.array([3, 4], np.uint32)}
    assert SO.differing_bits({k: v.copy() for k, v in plain.items()}, plain) == []
    got = {k: v.copy() for k, v in plain.items()}
    got["a"][1] = -0.0
    assert len(SO.differing_bits(got, plain)) == 1 and "a: 1 element(s)" in SO.differing_bits(got, plain)[0]
    got = {"a": plain["a"].copy()}
    assert SO.differing_bits(got, plain) != []
    got = {"a": plain["a"].copy(), "n": plain["n"].astype(np.uint64)}
    assert SO.differing_bits(got, plain) != []


def test_the_delay_respects_the_rule_it_was_sized_by():
    """at least 20 times the largest measured call of an ENQUEUES row, not under 50 ms, a few hundred ms at the most"""
    assert SO.MEASURED and set(SO.MEASURED) <= set(XC.ROWS)
    largest = max(ms for row, ms in SO.MEASURED.items() if SO.WAITS[row] == SO.ENQUEUES)
    assert max(50.0, 20.0 * largest) <= SO.DELAY_MS <= 400.0, (largest, SO.DELAY_MS)
