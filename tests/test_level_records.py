"""The engine's host side, characterised without a GPU: every Engine.run
call of tests/golden/make_level_records.py hands the library and the HIP
runtime the same launches with the same arguments, stages the same pack
bytes and returns the same results as tests/golden/level_records.json holds.
The fixture was written by the commit before the level records (_Plan,
_LevelOpts, _LevelState ...) existed and is not regenerated from later code:
a change of the engine's plumbing that moves a launch argument shows here."""
import importlib.util
import json
import os

import pytest

from hyperopt_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    spec = importlib.util.spec_from_file_location(
        "make_level_records", os.path.join(GOLDEN, "make_level_records.py"))
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

with open(os.path.join(GOLDEN, "level_records.json")) as f:
    RECORDS = json.load(f)


def test_records_have_declared_fields_only():
    """The plan, the options, the level / launch / slice records and the
    readback record: a field that was not declared raises on read and on
    write; a declared one that was not given reads as its default."""
    from hyperopt_amd import engine as E
    for cls in (E._LevelOpts, E._Plan, E._LevelState, E._LaunchState, E._GroupSlice,
                E._Readback):
        rec = cls()
        assert not hasattr(rec, "__dict__"), cls
        with pytest.raises(AttributeError):
            rec.no_such_field
        with pytest.raises(AttributeError):
            rec.no_such_field = 1
        if cls is not E._LevelOpts:
            with pytest.raises(AttributeError):
                cls(no_such_field=1)
    lv = E._LevelState(n_rows=3)
    assert lv.n_rows == 3 and lv.d_c32n is None and lv.o_rows is None
    with pytest.raises(AttributeError):
        lv.d_c32m  # (a misspelt pointer is an error, not a null pointer in a launch)
    assert E._LevelOpts().precision == 32 and E._LevelOpts(scorer="table").hooks is False


def test_every_case_is_recorded():
    assert M is not None, "libtpe_hip.so not loadable: %s" % globals().get("_WHY")
    assert sorted(RECORDS) == CASES


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_level_records(name):
    assert M is not None, "libtpe_hip.so not loadable"
    got, want = M.capture(name), RECORDS[name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g["launches"], w["launches"])):
            assert a == b, "call %d, launch %d" % (k, i)
        assert len(g["launches"]) == len(w["launches"]), "call %d" % k
        assert g == w, "call %d" % k
