"""What tests/test_gpu_exact_buffers.py rests on, checked without a GPU: the arena of tests/exact_buffers.py on CPU tensors, that
the table of tests/exact_buffers_cases.py names every device-pointer entry point of the headers, and that no kNN row of it rests
on an exact tie (DESIGN.md section 10 leaves those open)."""
import os
import re

import numpy as np
import pytest

import exact_buffers as EB
import exact_buffers_cases as XC
import handle_history_cases as HH

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arena():
    return EB.Arena("cpu", 1 << 20)


def test_addresses_have_the_promised_residues_and_payloads_their_exact_sizes():
    a = _arena()
    for i, (kind, length, misalign, want) in enumerate((("u8", 5, None, 1), ("u32", 7, None, 4), ("f32", 210, None, 4), ("u64", 3, None, 8), ("f64", 16, None, 8),
                                                        ("f32", 9, 0, 0), ("f32", 9, 8, 8), ("f32", 9, 12, 12), ("u8", 70, 3, 3), ("u32", 0, None, 4))):
        v = a.take("b%d" % i, length, kind, misalign)
        assert a.address("b%d" % i) % 16 == want, (kind, misalign)
        assert v.numel() == length and v.numel() * v.element_size() == a.buffers[-1][2] == length * EB.KINDS[kind][1]
        assert length == 0 or v.data_ptr() == a.address("b%d" % i)
        assert (v.contiguous().view(torch.uint8) == EB.FILL_BYTE).all()
    # guards of at least 16 KiB on either side of every payload, all of them 0xA5
    spans = sorted((first, first + n) for _name, first, n in a.buffers)
    assert spans[0][0] >= EB.GUARD and spans[-1][1] + EB.GUARD <= a.bytes.numel()
    assert all(b[0] - p[1] >= EB.GUARD for p, b in zip(spans, spans[1:]))
    a.check("fresh")


def test_an_input_holds_its_data_bit_for_bit():
    a = _arena()
    for data in (np.arange(7, dtype=np.uint32) * 0x01010101, np.array([[1.5, np.nan, -0.0]], np.float32), np.array([2 ** 63 + 5, 1], np.uint64),
                 np.array([np.pi], np.float64), np.array([1, 0, 255], np.uint8)):
        v = a.take("in", data.size, EB.kind_of(data), data=data)
        assert v.numpy().tobytes() == data.tobytes()
    a.check("inputs")


@pytest.mark.parametrize("kind", sorted(EB.KINDS))
def test_a_write_one_element_before_or_after_a_payload_is_reported_and_one_inside_is_not(kind):
    size = EB.KINDS[kind][1]
    for side in ("before", "after", "inside"):
        a = _arena()
        a.take("left neighbour", 33, "f32")
        v = a.take("the buffer", 10, kind)
        a.take("right neighbour", 33, "u64")
        first = a.address("the buffer") - a.base
        at = {"before": first - size, "after": first + 10 * size, "inside": first + 3 * size}[side]
        a.bytes[at:at + size] = 0
        if side == "inside":
            a.check(side)
            continue
        with pytest.raises(AssertionError) as e:
            a.check("planted")
        text = str(e.value)
        assert "'the buffer'" in text and side in text and "neighbour" not in text, text
        assert ("%d byte(s) %s" % (size if side == "before" else 1, side)) in text, text


def test_a_write_far_into_a_guard_is_reported_too():
    a = _arena()
    a.take("only", 4, "u32")
    a.bytes[a.address("only") - a.base + 16 + EB.GUARD - 1] = 1  # the last byte of the guard behind it
    with pytest.raises(AssertionError):
        a.check("far")


def test_untouched_looks_at_the_masked_elements_only():
    a = _arena()
    v = a.take("rows", 12, "f32").reshape(4, 3)
    v[1, 2] = 0.0
    mask = np.array([True, False, True, True])
    EB.Arena.untouched(v, mask, "other rows")
    EB.Arena.untouched(v.numpy(), mask, "as a numpy array")
    with pytest.raises(AssertionError):
        EB.Arena.untouched(v, np.array([False, True, False, False]), "the written row")
    with pytest.raises(AssertionError):
        EB.Arena.untouched(v, np.arange(12) == 5, "the written element")
    EB.Arena.untouched(v, np.arange(12) != 5, "every other element")
    b = a.take("flags", 9, "u8")
    b[8] = 1
    with pytest.raises(AssertionError):
        EB.Arena.untouched(b, np.arange(9) >= 8, "the written flag")


# ---- completeness -------------------------------------------------------------------------------------------------------------------------
def _declared():
    names = []
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if re.fullmatch(r"pcpx\w*\.h", f):
            names += re.findall(r"^int (pcpx_\w+_dev)\(", open(os.path.join(inc, f)).read(), re.M)
    return names


def test_every_device_pointer_entry_point_is_a_row():
    declared = _declared()
    assert len(declared) == len(set(declared)) >= 47
    covered = {s for r in XC.ROWS.values() for s in r.symbols}
    assert set(XC.EXTRA) <= set(declared)  # (the builds and pcpx_bounding_box_dev are declarations like the others)
    uncovered = sorted(set(declared) - covered - set(XC.EXEMPT))
    print("declared %d, covered %d, exempt %d, uncovered %d" % (len(declared), len(covered), len(XC.EXEMPT), len(uncovered)))
    assert uncovered == []
    assert sorted(covered - set(declared)) == []  # no row names a symbol that does not exist
    assert set(XC.EXEMPT) <= set(declared) and not covered & set(XC.EXEMPT)
    assert len(XC.EXEMPT) == 2


def test_every_row_has_a_family_and_names_the_test_that_pins_its_plain_form():
    for name, r in XC.ROWS.items():
        assert r.family in ("knn", "any", "free"), name
        assert set(XC.clouds_of(name)) <= set(XC.CLOUDS)
        if r.pinned is None:
            assert name == "bounding_box"  # (tests/test_gpu_exact_buffers.py compares it with numpy itself, part b)
            continue
        path, test = r.pinned.split("::")
        assert re.search(r"^def %s\(" % re.escape(test), open(os.path.join(ROOT, "tests", path)).read(), re.M), (name, r.pinned)


def test_the_clouds_are_the_ones_the_rows_need():
    s = {c: HH.statistics(c) for c in XC.CLOUDS}
    assert s["c70"]["groups"] == 2 and s["c70"]["n"] % HH.GROUP == 6 and s["c70"]["n"] % 4 == 2
    assert s["c5000g"]["n"] < s["c5000g"]["n_in"] and XC.KNN_CLOUDS == ("c70", "c1300")
    for c in XC.CLOUDS:  # the slices start at a group boundary and end inside a group, inside the cloud
        n = s[c]["n"]
        first, count = XC.slice_of(type("C", (), {"n": n}))
        assert first % HH.GROUP == 0 and (first + count) % HH.GROUP != 0 and first + count < n
    assert {k for k in XC.ALL_KS if k in (8, 16, 32)} == {8, 32} and (15, 16) in XC.PITCHES and 40 in XC.ALL_KS  # both whole-row forms, the passes
    assert {(12, 16), (3, 8)} <= set(XC.PITCHES)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud", XC.KNN_CLOUDS)
def test_no_knn_row_rests_on_a_tie(oracle, cloud):
    assert HH.knn_ties(oracle, cloud) == 0  # (every k of KS, over the self, batch and latency queries)
    pts = HH.inputs(cloud)["points"]
    k1 = min(max(XC.ALL_KS) + 1, len(pts))
    _idx, cnt, d2 = oracle.knn_bruteforce(pts, pts, k1, eps=XC.EPS, nthreads=16, want_d2=True)
    for k in XC.ALL_KS:  # (the k of the padded pitches as well)
        both = cnt > k
        assert int((d2[both, k - 1] == d2[both, k]).sum()) == 0, (cloud, k)
