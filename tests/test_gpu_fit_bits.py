"""The bits of the float64 fits against a recording (tests/golden/fit_bits.npz, written by tests/golden/make_fit_bits.py on the
commit before the sums of the rigid fit, the plane fit and the point-to-plane system moved into one shared reducer).  Every result
bit depends on the order of the additions -- a thread's items a grid stride apart in ascending order, the fixed tree over a block's
256 threads, the 64 blocks in block order -- and the cases (tests/fit_bits_cases.py) are the smallest sizes at which each part of
that order runs.  A CRC32 of every case's inputs comes first, so that a drift of the random generator reads "inputs differ" and is
not mistaken for a bit mismatch.  NaN outputs are compared by their bits like everything else."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import fit_bits_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "fit_bits.npz"))


def test_the_fixture_holds_every_case_and_nothing_else(fixture):
    assert sorted({k.split("/")[0] for k in fixture.files}) == sorted(Cs.CASES)
    assert os.path.getsize(os.path.join(GOLDEN, "fit_bits.npz")) < 256 * 1024


@pytest.mark.parametrize("name", Cs.CASES)
def test_fit_bits_equal_the_recording(pkg, fixture, name):
    pytest.importorskip("torch")
    assert np.array_equal(Cs.crc(name), fixture[name + "/crc"]), "inputs differ from the recording's: %s" % name
    got = Cs.run(pkg, name)
    assert sorted(got) == sorted(k.split("/", 1)[1] for k in fixture.files if k.startswith(name + "/") and not k.endswith("/crc"))
    for key, a in got.items():
        want = fixture[name + "/" + key]
        a = np.ascontiguousarray(a)
        print(name, key, a.reshape(-1)[:4].tolist())
        assert a.dtype == want.dtype and a.shape == want.shape, (name, key, a.dtype, want.dtype, a.shape, want.shape)
        assert np.array_equal(Cs.bits(a), Cs.bits(want)), (name, key, a.tolist(), want.tolist())
    if name == "fit_dev":  # the device forms with a count on the device equal the host forms over the same prefix
        for key in ("rigid", "rigid_rms", "plane", "plane_rms"):
            assert np.array_equal(Cs.bits(got[key]), Cs.bits(got["host_" + key])), key
    if name == "extract_planes":  # the dead rounds' entries are the zeros the call began with
        found = int(got["found"][0])
        assert found >= 1 and int(got["dev_count"][0]) == found and len(got["dev_planes"]) == found + 2
        assert not Cs.bits(got["dev_planes"])[found:].any() and not Cs.bits(got["dev_refits"])[found:].any() and not got["dev_scores"][found:].any()
        assert np.array_equal(Cs.bits(got["dev_refits"])[:found], Cs.bits(got["refits"]))
    if name == "icp_point":  # the loop stopped before max_iterations: the stopped rounds' fits saw a count word of zero
        import icp_model
        assert int(got["words"][0]) == icp_model.CONVERGED and 1 < int(got["words"][1]) < icp_model.RECOVERY_ITERATIONS
    if name == "icp_plane":
        assert int(got["words"][1]) == Cs.ICP_PLANE["iterations"] and int(got["words"][2]) > 16384  # (a thread of the sums has a second row)
