"""Host tables the ViT models' fused step is launched from, without a GPU: the rows of the W^T table (which Linear
weights get a transposed copy, where it lives) and the early all-reduce buckets of the data-parallel exchange.
tests/golden/vit_wt_buckets.json holds them as the code computed them before ViTSOM and ViTClassifier shared one base
class; each W^T row is [parameter name, src, off, N, K]."""
import copy
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN


def _expected(case):
    with open(os.path.join(GOLDEN, "vit_wt_buckets.json")) as f:
        return json.load(f)[case]


def _model(case):
    import bench
    import vit_som_amd
    if case == "c3_512":
        return vit_som_amd.ViTSOM(bench.c3_config(512), device="cpu")
    z = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    cls = vit_som_amd.ViTClassifier if case.startswith("ref_vitcls") else vit_som_amd.ViTSOM
    cfg = json.loads(str(z["config"] if "config" in z.files else z["config_json"]))
    return cls(copy.deepcopy(cfg), device="cpu")


def _wt_rows(m):
    name_at = {off: n for n, (off, _, _) in m.arena.offsets.items()}
    return [[name_at[r[0]]] + r for r in m._wt_table.tolist()]


@pytest.mark.parametrize("case", ["c3_512", "ref_vitcls_hd8", "ref_vitcls_hd32"])
def test_wt_table_and_buckets_are_pinned(case):
    m, ref = _model(case), _expected(case)
    assert _wt_rows(m) == ref["wt_table"]
    assert {k: list(v) for k, v in m._exchange_buckets().items()} == ref["buckets"]


def test_vitsom_classification_keeps_the_encoder_rows():
    # the encoder rows stay where they were; the decoder, whose gradients are zero in this mode, needs none
    m, ref = _model("ref_cls_tiny"), _expected("ref_cls_tiny")
    rows = _wt_rows(m)
    for r in ref["wt_table"]:
        assert r in rows, r[0]
    assert {k: list(v) for k, v in m._exchange_buckets().items()} == ref["buckets"]
