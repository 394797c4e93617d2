"""Every tensor argument of every evaluation wrapper of ops.py (the table in ops_arguments.py), on the device: the valid call
goes through to its entry, and each way of getting one argument wrong -- on the host, of the wrong dtype, strided, a row
or an element short, missing -- is a ValueError that names the argument, raised before the library is reached.

No kernel of the library runs: ops.lib is the recording stub throughout, so a check that is missing fails the test by
reaching the recorder and can never hand a host pointer or a short buffer to a kernel."""
import pytest
import torch

import ops_arguments as A
from vit_som_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture
def stub(monkeypatch):
    s = A.StubLib()
    monkeypatch.setattr(ops, "lib", s)
    return s


def _strided(t):
    """The shape of t over every second element of a buffer twice as wide: innermost stride 2."""
    return t.new_zeros(*t.shape[:-1], 2 * t.shape[-1])[..., ::2]


def mutations(arg, t):
    """(what, value) for every wrong form of the valid tensor t of an argument of this kind."""
    yield "a host copy", t.cpu()
    if arg.dtype is not None:
        yield "a wrong dtype", t.to(A.WRONG[arg.dtype])
    strided = _strided(t)
    if not strided.is_contiguous():                              # a tensor of one element has no other layout
        yield ("innermost stride 2" if arg.kind == A.MATRIX else "a non-contiguous view"), strided
    if arg.sized:
        yield "one row or element short", t[:-1]
    if not arg.optional:
        yield "None", None


@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_every_argument_is_checked_before_the_library(stub, row):
    valid = row.make(DEV)
    if not row.reads_back:
        row.fn(**valid)
        assert stub.calls == [row.entry]
    for name, arg in row.args.items():
        for what, value in mutations(arg, valid[name]):
            stub.calls.clear()
            with pytest.raises(ValueError, match=rf"^{name}\b"):       # every message opens with the argument's name
                row.fn(**{**valid, name: value})
            assert stub.calls == [], f"{row.name}: {name} as {what} reached {stub.calls}"
        if arg.optional and not row.reads_back:
            stub.calls.clear()
            row.fn(**{**valid, name: None, **{other: None for other in arg.together}})
            assert stub.calls == [row.entry], f"{row.name}: {name}=None"
