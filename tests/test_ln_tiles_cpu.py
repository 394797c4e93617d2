"""Host checks of vsom_set_ln_tiles (the 192 x 192 tiles of the LayerNorm-fused input-gradient GEMM): the setting takes
part in the launch-tape key, and only 0 and 1 are accepted.  No launch happens."""
import types


def test_set_ln_tiles_rejects_unknown_modes():
    from vit_som_amd._lib import last_error, lib
    for bad in (2, -1, 3):
        assert lib.vsom_set_ln_tiles(bad) == -1
        assert "set_ln_tiles" in last_error()
    assert lib.vsom_set_ln_tiles(0) == 0
    assert lib.vsom_set_ln_tiles(1) == 0


def test_partial_layout_does_not_depend_on_the_setting():
    from vit_som_amd import ops
    from vit_som_amd._lib import lib
    try:
        sizes = []
        for mode in (0, 1):
            ops.set_ln_tiles(mode)
            sizes.append([lib.vsom_linear_bwd_input_ln_partial_bytes(M, 192) for M in (33280, 33280 + 17, 2048, 4165)])
        assert sizes[0] == sizes[1] == [520 * 2 * 192 * 4, 521 * 2 * 192 * 4, 32 * 2 * 192 * 4, 66 * 2 * 192 * 4]
    finally:
        ops.set_ln_tiles(1)


def test_ln_tiles_is_part_of_the_tape_key(monkeypatch):
    from vit_som_amd import ops
    from vit_som_amd.step import _StepTape
    monkeypatch.setattr(ops, "stream", lambda: 0)
    m = types.SimpleNamespace(world_size=1, _use_vsom_comm=False)
    try:
        assert ops.get_ln_tiles() == 1                                     # default: the 192 x 192 tiles
        k1 = _StepTape._key(m)
        ops.set_ln_tiles(0)
        assert ops.get_ln_tiles() == 0
        k0 = _StepTape._key(m)
        assert k0 != k1
        ops.set_ln_tiles(1)
        assert _StepTape._key(m) == k1
    finally:
        ops.set_ln_tiles(1)
