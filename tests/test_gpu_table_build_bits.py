"""k_table_build's output, byte for byte, against fixtures recorded on an
MI355X (tools/record_table_bits.py, tests/golden/table_bits/).

The build's sums are ordered: per lane the items it, it + stride, ..., then
the row's lanes, then (cooperative labels) the block's waves.  A change to
the item loop that keeps every sum's terms, order and roundings leaves every
byte the build writes where it was; anything else moves some.  Compared per
case: the cell records, the (m_below, m_above) pairs, the score cells
k_table_score derives from them and the job's tpe_table record.

Each case asserts the properties it is there for from the plan read back
(tests/table_bits_cases.py restates the windows and the per-lane scale walk
on the CPU):

  coop-partial   nb <= kCoopCells (a quad per block), nb % 4 != 0
  wave-partial   nb >  kCoopCells (a quad per wave), nb % 4 != 0
  coop-natural   a natural history's table, wide list not empty
  gap            quads with an odd window length, with fewer than 16 items
                 and with an empty window; wide list not empty
  late-rescale   lanes that meet a term over 2^8 above the scale they had
                 already set (one cluster of duplicates late in sorted order)
"""
import numpy as np
import pytest

from tests import table_bits_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    return Engine()


@pytest.mark.parametrize("name", list(C.CASES))
def test_build_bits(engine, name):
    T = C.build(engine, name)
    P = C.properties(T)
    print("table bits: %-13s %s" % (name, P))
    C.check_properties(name, P)
    # the restated windows are the kernel's: its deepest walk is theirs
    if not T.replanned:
        assert int(T.tab["build_items"]) == P["max_items"], (T.tab["build_items"], P["max_items"])
    want = np.load(C.fixture_path(name))
    assert int(np.frombuffer(want["table"].tobytes(), T.tab.dtype)[0]["nb"]) == T.nb
    got = C.parts(T)
    for part in C.PARTS:
        a, b = got[part], want[part]
        assert a.size == b.size, (name, part, a.size, b.size)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (name, part, "first differing byte", int(bad[0]), "of", a.size,
                               "differing", bad.size)
