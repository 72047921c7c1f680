"""Record the fixture of tests/test_gpu_joint_bits.py on a GPU: what the joint
scorers (tpe_joint_score, tpe_joint_score_rows, tpe_joint_chain_rows_keep), a
grid-pool joint score and a ``loo_label_curves`` curve give on every case of
that file, doubles as uint64, as tests/golden/joint_score_bits.npz.

    python tools/record_joint_bits.py            # write the fixture
    python tools/record_joint_bits.py --compare  # compare with the recorded one, write nothing

Run it at the commit whose bits are the reference (the parent of a change
that must not move them).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import test_gpu_joint_bits as C  # noqa: E402


def main(compare):
    got = {}
    for case in C.CASES:
        part = C.parts(case)
        got.update(part)
        print(case, "arrays", len(part), "values", sum(a.size for a in part.values()), flush=True)
    if not compare:
        np.savez_compressed(C.GOLDEN, **got)
        print("wrote %s (%d bytes)" % (C.GOLDEN, os.path.getsize(C.GOLDEN)))
        return 0
    differ = 0
    with np.load(C.GOLDEN) as want:
        differ += sorted(want.files) != sorted(got)
        for name in sorted(got):
            same = name in want.files and got[name].tobytes() == want[name].tobytes()
            differ += not same
            print("  %-36s %6d  %s" % (name, got[name].size, "same" if same else "DIFFERS"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main("--compare" in sys.argv[1:]))
