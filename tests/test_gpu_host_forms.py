"""The outputs of the handle family's host-pointer forms and of their _dev forms against a recording (tests/golden/host_forms.npz,
written by tests/golden/make_host_forms.py on the commit before these forms moved to one staging helper and their scratch layouts to
Carve).  Every output is deterministic and is compared by its bits; the cases (tests/host_forms_cases.py) are the smallest clouds
at which each path of the staging and of the layouts runs.  A CRC32 of every case's inputs comes first, so that a drift of the
random generator reads "inputs differ" and is not mistaken for a mismatch.  The recording holds every optional output; every other
subset of them is then asked of both forms, and what is asked must equal the recording: an offset that depends on which outputs
exist shows there."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import host_forms_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "host_forms.npz"))


def test_the_fixture_holds_every_case_and_nothing_else(fixture):
    assert sorted({k.split("/")[0] for k in fixture.files}) == sorted(Cs.CASES)
    assert os.path.getsize(os.path.join(GOLDEN, "host_forms.npz")) < 256 * 1024


def _equal(name, form, ask, got, fixture):
    for key, a in got.items():
        want = fixture[name + "/" + key]
        a = np.ascontiguousarray(a)
        assert a.dtype == want.dtype and a.shape == want.shape, (name, form, sorted(ask), key, a.dtype, want.dtype, a.shape, want.shape)
        assert np.array_equal(Cs.bits(a), Cs.bits(want)), (name, form, sorted(ask), key, a.tolist(), want.tolist())


@pytest.mark.parametrize("name", Cs.CASES)
def test_both_forms_equal_the_recording(pkg, fixture, name):
    pytest.importorskip("torch")
    assert np.array_equal(Cs.crc(name), fixture[name + "/crc"]), "inputs differ from the recording's: %s" % name
    op = Cs.split(name)[1]
    recorded = sorted(k.split("/", 1)[1] for k in fixture.files if k.startswith(name + "/") and not k.endswith("/crc"))
    assert recorded == sorted(Cs.OUTPUTS[op][0] + Cs.OUTPUTS[op][1])
    count = int(fixture[name + "/count"][0]) if "count" in recorded else None
    for form, run in (("host", Cs.run_host), ("dev", Cs.run_dev)):
        for i, ask in enumerate(Cs.asks(op, form == "dev")):
            got = run(pkg, name, ask) if form == "host" else run(pkg, name, ask, count)
            if got is None:  # (a batch form has no _dev form)
                break
            assert sorted(got) == sorted(Cs.OUTPUTS[op][0] + tuple(ask)), (name, form, sorted(ask), sorted(got))
            assert i > 0 or sorted(got) == recorded
            _equal(name, form, ask, got, fixture)
