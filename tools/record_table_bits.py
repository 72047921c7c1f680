"""Record the fixtures of tests/test_gpu_table_build_bits.py on a GPU: what
tpe_table_build wrote for every case of tests/table_bits_cases.py (cell
records, (m_below, m_above) pairs, score cells, tpe_table record), as
tests/golden/table_bits/<case>.npz.

    python tools/record_table_bits.py            # write the fixtures
    python tools/record_table_bits.py --compare  # compare with the recorded ones, write nothing

Run it at the commit whose bits are the reference (the parent of a change
that must not move them).  Each case's properties are printed and checked
before anything is written.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import table_bits_cases as C  # noqa: E402


def main(compare):
    from hyperopt_amd.engine import Engine
    eng = Engine()
    os.makedirs(C.GOLDEN, exist_ok=True)
    differ = 0
    for name in C.CASES:
        T = C.build(eng, name)
        P = C.properties(T)
        print(name, P, "build_items", int(T.tab["build_items"]), flush=True)
        C.check_properties(name, P)
        got = C.parts(T)
        if compare:
            want = np.load(C.fixture_path(name))
            for k in C.PARTS:
                same = got[k].tobytes() == want[k].tobytes()
                differ += not same
                print("  %-12s %8d bytes  %s" % (k, got[k].size, "same" if same else "DIFFERS"))
        else:
            np.savez_compressed(C.fixture_path(name), **got)
            print("  wrote %s (%d bytes)" % (C.fixture_path(name),
                                            os.path.getsize(C.fixture_path(name))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main("--compare" in sys.argv[1:]))
