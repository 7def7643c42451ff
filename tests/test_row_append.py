"""The matrix the DEVICE holds after rows were appended (csrc/engine.hip append_rows_on_device, csrc/cuts.inc k_csc_append_rows).

Solution::add_constraint is add_constraints of one row: one host path, one re-layout of the device CSC.  The other tests see the device
CSC only through the pivots that follow an append; here it is read back (state keys dev_csc_* / dev_csr_*) and compared, exactly, with the
column-major form of the host's CSR mirror: old entries keep their order, a new entry goes to the end of its column (its row index is the
largest), the slack columns come last.  Integer arrays with array_equal, values byte for byte."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from tests.test_cut_rounds import _model, _pending, _solved_with_pending_terms

pytestmark = pytest.mark.gpu
DEV_KEYS = ("dev_csc_indptr", "dev_csc_indices", "dev_csc_data", "dev_csr_indptr", "dev_csr_data")


def _device_matrix_is_the_mirror(s):
    """Asserts that the device CSC / CSR are the host mirror's matrix; returns the bytes of the five device arrays."""
    indptr = s.state("csr_indptr").astype(np.int64)
    indices = s.state("csr_indices").astype(np.int64)
    data = s.state("csr_data")
    m = len(indptr) - 1
    N = s.num_vars + m                                   # one slack per row
    assert len(indices) == len(data) == indptr[-1]
    rows = np.repeat(np.arange(m), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    cptr = np.r_[0, np.cumsum(np.bincount(indices, minlength=N))]
    csc_rows = rows[order]
    csc_vals = data[order]
    dev = {k: s.state(k) for k in DEV_KEYS}
    assert np.array_equal(dev["dev_csc_indptr"].astype(np.int64), cptr)
    assert np.array_equal(dev["dev_csc_indices"].astype(np.int64), csc_rows)
    assert dev["dev_csc_data"].tobytes() == csc_vals.tobytes()
    assert np.array_equal(dev["dev_csr_indptr"].astype(np.int64), indptr)
    assert dev["dev_csr_data"].tobytes() == data.tobytes()
    return tuple(dev[k].tobytes() for k in DEV_KEYS)


def _box_problem(n, rows):
    """Maximize sum (1 + j / 8) x_j over x in [0, 1]^n under `rows` [(expr, rhs)], all <=."""
    p = M.Problem(M.MAXIMIZE)
    p.add_vars_bulk(1.0 + np.arange(n) / 8.0, np.zeros(n), np.ones(n))
    for expr, rhs in rows:
        p.add_constraint(expr, M.LE, rhs)
    return p


def _append_both_ways(s, rows, batch=None):
    """`rows` one by one on a clone, `batch` (default: the same rows) in one call on another: both hold the mirror's matrix, the same
    device bytes and the same model.  Returns the two solutions."""
    a, b = s.clone(), s.clone()
    for expr, op, rhs in rows:
        a = a.add_constraint(expr, op, rhs)
        _device_matrix_is_the_mirror(a)
    b = b.add_constraints(rows if batch is None else batch)
    assert _device_matrix_is_the_mirror(a) == _device_matrix_is_the_mirror(b)
    assert _model(a) == _model(b)
    return a, b


def test_tiny_model_with_an_empty_column():
    # variable 5 is in no row: its column is empty; rhs = 10 is never reached on [0, 1]^6, so no append is followed by a pivot
    s = _box_problem(6, [([(0, 1.0), (1, 2.0), (2, 0.5)], 2.0), ([(2, 1.5), (3, 2.0), (4, 1.0)], 2.5)]).solve()
    _device_matrix_is_the_mirror(s)
    rows = [([(5, 1.25)], M.LE, 10.0),                                           # the empty column only
            ([(0, 0.75), (5, 2.5)], M.LE, 10.0),                                 # the first and the last column
            ([(j, 1.0 + j / 4.0) for j in range(6)], M.LE, 10.0),                # all six
            ([(3, 3.0)], M.LE, 10.0)]                                            # one middle column
    it0 = s.clone().stats()["iterations"]
    a, b = _append_both_ways(s, rows, batch=rows[:2] + [([], M.LE, 10.0)] + rows[2:])
    assert a.stats()["iterations"] == b.stats()["iterations"] == it0
    assert len(a.state("csr_indptr")) - 1 == len(b.state("csr_indptr")) - 1 == 6
    # the constraint without terms has no row (constraint -> row is -1): it is counted as a constraint, and its dual value is 0
    assert a.num_constraints == 6 and b.num_constraints == 7 and b.cut_info()["rows_without_terms"] == 1
    assert len(a.dual_values()) == 6 and len(b.dual_values()) == 7 and b.dual_values()[4] == 0.0


def test_a_column_longer_than_the_copy_group():
    # 40 rows hold variable 0: 16 lanes copy a column, so the stride loop over its entries runs three trips
    base = [([(0, 1.0 + i / 64.0), (1 + i % 2, 2.0)], 50.0 + i) for i in range(40)]
    s = _box_problem(3, base).solve()
    _device_matrix_is_the_mirror(s)
    _append_both_ways(s, [([(0, 7.0), (2, 0.5)], M.LE, 100.0), ([(0, 9.0)], M.LE, 100.0)])


def test_columns_on_both_sides_of_a_scan_tile():
    # N + 1 = 4203 > 4096: the per-column counts of a round span two tiles of the scan
    n = 4200
    base = [([(j, 1.0 + (j % 5) / 4.0) for j in range(0, n, 7)], 1e4), ([(j, 2.0) for j in range(3, n, 11)], 1e4)]
    s = _box_problem(n, base).solve()
    _device_matrix_is_the_mirror(s)
    rows = [([(0, 1.5), (4095, 2.5), (4096, 3.5), (4199, 4.5)], M.LE, 1e4), ([(4095, 0.25), (4096, 0.75)], M.LE, 1e4)]
    a, b = _append_both_ways(s, rows)
    for t in (a, b):                                                             # again, singly, on the re-laid-out result
        t = t.add_constraint([(0, 5.0), (4095, 6.0), (4096, 7.0), (4199, 8.0)], M.LE, 1e4)
        _device_matrix_is_the_mirror(t)


def _cut_a_basic_value(s, skip=()):
    """One single append that is followed by dual pivots: a bound row below the value of a variable."""
    x = s.values()
    j = next(int(j) for j in np.argsort(x)[::-1] if int(j) not in skip)
    assert x[j] > 1e-3
    return s.add_constraint([(j, 0.7)], M.LE, float(x[j]) * 0.35)


def test_on_the_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")                                        # (the set-up of test_cut_rounds.test_compact_factor)
    s = lpgen.build_problem(M.Problem, lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)).solve()
    assert s.stats()["factor_active"] == 1
    _device_matrix_is_the_mirror(_cut_a_basic_value(s))


def test_with_pending_low_rank_terms(monkeypatch):
    monkeypatch.setenv("MLP_LOWRANK", "3")                                       # (test_cut_rounds.test_pending_terms_of_the_delayed_update_mode)
    s, _, bounded = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    assert _pending(s) > 0
    _device_matrix_is_the_mirror(_cut_a_basic_value(s, skip=bounded))
