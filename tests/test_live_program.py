"""Domain.live_program: the space's liveness as clauses over its selectors
agrees with ``reachable`` (the definition) on every selector assignment; its
CSR form, interpreted in numpy, agrees with ``reachable`` row by row; and the
entry points of csrc/tpe_sampled.hip report argument errors before any GPU
call."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, hp
from hyperopt_amd import _lib as L
from hyperopt_amd import pool as pool_mod
from tests import cond_util as C
from tests.golden import spaces

SPACES = {name: spaces.SPACES[name] for name in ("readme", "nested", "mixed_50d", "many_dists")}
SPACES.update(C.CRAFTED)
FLAT = ("mixed_50d", "many_dists")


def _domain(name):
    return Domain(lambda x: 0, SPACES[name](hp))


@pytest.mark.parametrize("name", sorted(SPACES))
def test_program_matches_reachable(name):
    domain = _domain(name)
    prog = domain.live_program()
    if name == "expr_selector":
        assert prog is None
        return
    assert list(prog) == list(domain.params)
    assert domain.live_program() is prog  # cached
    n = 0
    for a in C.assignments(domain):
        assert C.program_live(prog, a) == C.walk_live(domain, a), a
        n += 1
    assert n >= 1
    if name in FLAT:
        assert all(cl == ((),) for cl in prog.values())
    for lab, clauses in prog.items():
        assert len(set(clauses)) == len(clauses), lab  # deduplicated
        if () in clauses:
            assert clauses == ((),), lab
        for c in clauses:  # no clause names a selector twice
            assert len({s for s, _ in c}) == len(c), (lab, c)


def test_program_forms():
    """The clauses themselves, where the rule's cases show."""
    prog = _domain("shared_node").live_program()
    assert prog["a"] == ((),)
    assert prog["x"] == ((("a", 0),), (("a", 1),), (("a", 2), ("b", 0)))
    assert prog["b"] == ((("a", 2),),)
    assert prog["z"] == ((("a", 2), ("b", 1)),)
    prog = _domain("selector_twice").live_program()
    assert prog["i0"] == ((("s", 0),),) and prog["i1"] == ((("s", 1),),)  # no (s=0, s=1)
    prog = _domain("pchoice_nested").live_program()
    assert prog["c"] == ((("p", 0),),) and prog["l"] == ((("p", 0), ("c", 1)),)
    assert prog["r"] == ((("p", 1),),)
    # a randint(low, high) selector: no program
    d = Domain(lambda x: 0, C.scope.switch(hp.randint("k", 1, 3), 0, hp.uniform("u", 0, 1),
                                           hp.uniform("v", 0, 1)))
    assert d.live_program() is None


@pytest.mark.parametrize("name", sorted(n for n in SPACES if n != "expr_selector"))
def test_csr_interpreter_matches_reachable(name):
    domain = _domain(name)
    labels = list(domain.params)
    label_off, clause_off, terms = pool_mod.program_csr(domain)
    assert label_off.dtype == clause_off.dtype == np.int32
    assert terms.dtype == L.COND_TERM_DTYPE and L.COND_TERM_DTYPE.itemsize == 8
    assert label_off[0] == clause_off[0] == 0 and clause_off[-1] == len(terms)
    rng = np.random.RandomState(len(labels))
    n = 257
    cols = C.random_columns(domain, n, rng, ld=n + 7)
    active = C.interpret(label_off, clause_off, terms, cols, n)
    sel = list(C.selector_ranges(domain))
    for r in range(n):
        decided = {lab: int(cols[labels.index(lab), r]) for lab in sel}
        want = set(domain.reachable(decided))
        assert {labels[j] for j in np.flatnonzero(active[:, r])} == want, r
    # the host path Pool.sample takes without a program gives the same mask
    sv = np.stack([cols[labels.index(lab), :n] for lab in sel], 1) if sel else np.zeros((n, 0))
    np.testing.assert_array_equal(pool_mod._host_active(domain, labels, sel, sv), active.T)


def test_program_csr_without_program():
    assert pool_mod.program_csr(_domain("expr_selector")) is None


def _program(n_labels=3, terms=((0, 1),)):
    """A program whose last label has one clause holding ``terms``."""
    label_off = np.zeros(n_labels + 1, np.int32)
    label_off[-1] = 1
    clause_off = np.asarray([0, len(terms)], np.int32)
    t = np.zeros(len(terms), L.COND_TERM_DTYPE)
    for i, (c, v) in enumerate(terms):
        t[i] = (c, v)
    return label_off, clause_off, t


def test_sampled_entry_points_argument_errors():
    """tpe_rows_active / tpe_pool_ranges / tpe_pool_take: a negative size, null
    pointers, an over-limit program and a term column outside [0, n_labels)
    are reported before any GPU call."""
    lib = L.load()
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch
    sizes = (ctypes.c_int32 * 1)()
    assert lib.tpe_sampled_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 1) == 1
    assert sizes[0] == L.COND_TERM_DTYPE.itemsize

    def rows_active(prog, n_rows=10, ld=16, n_labels=None, vals=one, active=one, n_active=one):
        lo, co, t = prog
        return lib.tpe_rows_active(vals, ld, n_rows, len(lo) - 1 if n_labels is None else n_labels,
                                   lo.ctypes.data, co.ctypes.data, t.ctypes.data, len(t), active,
                                   n_active, None)
    ok = _program()
    assert rows_active(ok, n_rows=0) == 0  # nothing to do
    assert lib.tpe_rows_active(None, 0, 5, 0, None, None, None, 0, None, None, None) == 0
    assert rows_active(ok, n_rows=-1) == -1 and b"tpe_rows_active" in lib.tpe_last_error()
    assert rows_active(ok, ld=-2) == -1
    assert lib.tpe_rows_active(one, 16, 10, 3, None, None, None, 0, one, one, None) == -1
    assert b"null pointer" in lib.tpe_last_error()
    for missing in ("vals", "active", "n_active"):
        assert rows_active(ok, **{missing: None}) == -1, missing
        assert b"null pointer" in lib.tpe_last_error()
    assert rows_active(ok, n_rows=17) == -1 and b"ld" in lib.tpe_last_error()
    for col in (-1, 3):
        assert rows_active(_program(terms=((col, 0),))) == -1
        assert b"column" in lib.tpe_last_error()
    assert rows_active(_program(n_labels=L.COND_MAX_LABELS + 1)) == L.E_UNSUPPORTED
    assert b"limit" in lib.tpe_last_error()
    assert rows_active(_program(terms=((0, 0),) * (L.COND_MAX_TERMS + 1))) == L.E_UNSUPPORTED
    many = np.zeros(3, np.int32)  # too many clauses (all empty)
    many[1:] = L.COND_MAX_CLAUSES + 1
    big = (many, np.zeros(L.COND_MAX_CLAUSES + 2, np.int32), np.zeros(0, L.COND_TERM_DTYPE))
    assert rows_active(big) == L.E_UNSUPPORTED
    bad = _program()
    bad[1][1] = 5  # clause_off does not end at n_terms
    assert rows_active(bad) == -1 and b"clause_off" in lib.tpe_last_error()

    pos = np.zeros(4, np.uint8)
    pp = pos.ctypes.data

    def ranges(n_rows=10, ld=16, n_labels=4, vals=one, active=one, positive=pp, out=one):
        return lib.tpe_pool_ranges(vals, active, ld, n_rows, n_labels, positive, out, None)
    assert ranges(n_labels=0) == 0
    assert ranges(n_rows=-1) == -1 and b"tpe_pool_ranges" in lib.tpe_last_error()
    assert ranges(n_labels=-1) == -1
    for missing in ("vals", "active", "positive", "out"):
        assert ranges(**{missing: None}) == -1, missing
        assert b"null pointer" in lib.tpe_last_error()
    assert ranges(n_rows=17) == -1 and b"ld" in lib.tpe_last_error()

    def take(k=3, ld=16, n_labels=4, vals=one, active=one, rows=one, out_v=one, out_a=one):
        return lib.tpe_pool_take(vals, active, ld, n_labels, rows, k, out_v, out_a, None)
    assert take(k=0) == 0 and take(n_labels=0) == 0
    assert take(k=-1) == -1 and b"tpe_pool_take" in lib.tpe_last_error()
    assert take(ld=-1) == -1 and take(n_labels=-2) == -1
    for missing in ("vals", "active", "rows", "out_v", "out_a"):
        assert take(**{missing: None}) == -1, missing
        assert b"null pointer" in lib.tpe_last_error()
