"""The search algorithms' host side, characterised without a GPU: every case
of tests/golden/make_suggest_records.py hands Engine.run, the prior kernel
and the anneal kernel the same work with the same keys and options, and
returns the same trial documents (dict key order included), as
tests/golden/suggest_records.json holds.  The fixture was written by the
commit before hyperopt_amd/walk.py existed and is not regenerated from later
code: a change of the level walk, the decode rule, the document builder or a
WorkBatch key shows here."""
import importlib.util
import json
import os

import pytest

from hyperopt_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    spec = importlib.util.spec_from_file_location(
        "make_suggest_records", os.path.join(GOLDEN, "make_suggest_records.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


try:
    L.load()
    M = _load()
    CASES = sorted(M.CASES)
except Exception as e:  # pragma: no cover - the build check covers this
    M, CASES = None, []
    _WHY = str(e)

with open(os.path.join(GOLDEN, "suggest_records.json")) as f:
    RECORDS = json.load(f)


def test_every_case_is_recorded():
    assert M is not None, "libtpe_hip.so not loadable: %s" % globals().get("_WHY")
    assert sorted(RECORDS) == CASES


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_suggest_records(name):
    assert M is not None, "libtpe_hip.so not loadable"
    got, want = M.capture(name), RECORDS[name]
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, "call %d" % i
        assert json.dumps(a) == json.dumps(b), "call %d: key order" % i
    assert len(got["calls"]) == len(want["calls"])
    assert got["docs"] == want["docs"]
    assert json.dumps(got["docs"]) == json.dumps(want["docs"])  # (dict key order too)


def test_study_record_has_declared_fields_only():
    """tpe's per-study record: a misspelt field raises on read and on write."""
    from hyperopt_amd import tpe
    st = tpe._Study.__new__(tpe._Study)
    assert not hasattr(st, "__dict__")
    with pytest.raises(AttributeError):
        st.no_such_field
    with pytest.raises(AttributeError):
        st.no_such_field = 1
