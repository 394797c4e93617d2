"""The evaluation wrappers of ops.py refuse host tensors before anything reaches the library, with ValueError (so under
`python -O` too), and the table in ops_arguments.py covers every wrapper of the range.  No GPU: ops.lib is the recording
stub, and a call that got past the checks would show in its record."""
import ast
import inspect

import pytest
import torch

import ops_arguments as A
from vit_som_amd import ops

SOURCE = inspect.getsource(ops)
FIRST, LAST = A.in_scope_range(SOURCE)


@pytest.fixture
def stub(monkeypatch):
    s = A.StubLib()
    monkeypatch.setattr(ops, "lib", s)
    return s


@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_host_tensors_are_refused_before_the_library(stub, row):
    with pytest.raises(ValueError, match="expected a HIP device tensor"):
        row.fn(**row.make("cpu"))
    assert stub.calls == []


def _functions():
    return [n for n in ast.parse(SOURCE).body if isinstance(n, ast.FunctionDef) and FIRST < n.lineno < LAST]


def test_no_assert_is_left_in_the_range():
    assert LAST - FIRST > 500
    left = [(f.name, n.lineno) for f in _functions() for n in ast.walk(f) if isinstance(n, ast.Assert)]
    assert left == []


def test_the_feature_named_helpers_are_gone():
    for name in ("_kmeans_x", "_pca_vec", "_pca_f64", "_probe_f64", "_probe_labels", "_tsne_y", "_gmm_kd", "_lbfgs_args"):
        assert not hasattr(ops, name), name
    for name in ("_f32", "_rows", "_matrix", "_dense", "_buffer"):
        assert callable(getattr(ops, name)), name


def test_the_table_names_every_wrapper_of_the_range():
    public = {f.name for f in _functions() if not f.name.startswith("_")}
    covered = {r.name.split("[")[0] for r in A.ROWS}
    assert covered.isdisjoint(A.EXEMPT)
    assert public - covered - A.EXEMPT == set(), "a wrapper without a row in ops_arguments.py (or a line in EXEMPT)"
    assert (covered | A.EXEMPT) - public == set(), "ops_arguments.py names functions the range does not have"
    for r in A.ROWS:                                             # every tensor argument of a row is one of its parameters
        made = r.make("cpu")
        assert set(made) <= set(inspect.signature(r.fn).parameters), r.name
        assert {k for k, v in made.items() if isinstance(v, torch.Tensor)} == set(r.args), r.name
