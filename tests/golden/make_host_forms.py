"""Writes tests/golden/host_forms.npz: the outputs of every case of tests/host_forms_cases.py from the host-pointer forms on the GPU,
every optional output asked, and a CRC32 of each case's inputs.  Only the public Python API is called, so the script runs unchanged
on any commit that has the entry points; the fixture in the repository was recorded on the commit before the handle family's host
forms moved to one staging helper and their scratch layouts to Carve.

    python tests/golden/make_host_forms.py [output.npz]
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import host_forms_cases as Cs  # noqa: E402


def main(path):
    pkg = importlib.import_module("point-cloud-processing_amd")
    out = {}
    for name in Cs.CASES:
        out[name + "/crc"] = Cs.crc(name)
        for key, a in Cs.run_host(pkg, name).items():
            out[name + "/" + key] = np.ascontiguousarray(a)
        print(name, "crc %08x" % int(out[name + "/crc"][0]), {k.split("/")[1]: np.asarray(v).shape for k, v in out.items() if k.startswith(name + "/")})
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "host_forms.npz"))
