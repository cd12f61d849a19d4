"""Regenerates tests/golden/ref_maps.npz and ref_assembly.npz from the reference's own host arithmetic: runs oracle/_ref/record (the
reference's unmodified objects under our main, oracle/ref_record.c; built by `make -C oracle ref REFERENCE=<tree>`) over the case lists of
tests/ref_fixtures.py.  The files hold numbers only.  tests/test_reference_fixtures_cpu.py reruns this where the recorder exists and requires
the committed arrays bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ref_fixtures as RF  # noqa: E402

LIMIT = 1000000     # bytes per committed file


def main():
    if not os.path.exists(RF.RECORD):
        sys.exit(f"{RF.RECORD} is not built: make -C oracle ref REFERENCE=<the reference tree>")
    for path, arrays in ((RF.MAPS_NPZ, RF.build_maps()), (RF.ASSEMBLY_NPZ, RF.build_assembly())):
        for k, a in arrays.items():
            assert a.dtype in (np.int32, np.float64), (k, a.dtype)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"{os.path.relpath(path, RF.ROOT)}: {len(arrays)} arrays, {size} bytes")
        assert size < LIMIT, f"{path}: {size} bytes: drop the largest npts of the list (never a -map style, a rank count or a mesh)"


if __name__ == "__main__":
    main()
