"""Record the fixture of tests/test_gpu_liar_bits.py on a GPU: the rows,
``S_at_pick`` and ``S_k`` (doubles as uint64) of ``liar_device``,
``liar_tree_device`` and ``liar_chain_device`` on every case of that file, as
tests/golden/liar_bits.npz.

    python tools/record_liar_bits.py            # write the fixture
    python tools/record_liar_bits.py --compare  # compare with the recorded one, write nothing

Run it at the commit whose bits are the reference (the parent of a change
that must not move them).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import test_gpu_liar_bits as C  # noqa: E402


def main(compare):
    got = {}
    for case in C.CASES:
        got.update(C.parts(*case))
        print(C.case_id(*case), "picks", got[C.case_id(*case) + "/rows"].size, flush=True)
    if not compare:
        np.savez_compressed(C.GOLDEN, **got)
        print("wrote %s (%d bytes)" % (C.GOLDEN, os.path.getsize(C.GOLDEN)))
        return 0
    differ = 0
    with np.load(C.GOLDEN) as want:
        for name in sorted(got):
            same = got[name].tobytes() == want[name].tobytes()
            differ += not same
            print("  %-36s %6d  %s" % (name, got[name].size, "same" if same else "DIFFERS"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main("--compare" in sys.argv[1:]))
