"""A stopped run resumes bit for bit: the oracle of every case is the uninterrupted run of the same model on the same inputs
(tests/resume.py), compared with torch.equal; the optimizer's semantics are held against torch.optim.AdamW by
test_ops_gpu.py::test_adamw_step's rule.  Shapes: the tiny goldens, and the depth-3 B = 192 config where the BMU pass has
to take the planes form."""
import functools

import pytest
import torch

import resume as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 8                      # steps of the uninterrupted run; stopped after STOP
STOP = 4


@functools.lru_cache(maxsize=None)
def _inputs(kind, sizes):
    return R.inputs_of(R.case(kind), list(sizes))


@functools.lru_cache(maxsize=None)
def _uninterrupted(kind, mode):
    """Run A, once per (model, mode): N steps, the tape recorded at step 3 and replayed after.  Read-only for its users."""
    c = R.case(kind)
    inputs = _inputs(kind, (c.batch,) * N)
    model, opt, sched = R.fresh(c, DEV)
    trace = R.run_steps(model, opt, sched, inputs, 1, N, mode)
    return trace, R.final_state(model, inputs[0])


def _no_differences(a, b, steps):
    for i in steps:
        bad = R.differences(a[i], b[i])
        assert not bad, (i, bad, {k: (a[i].get(k), b[i].get(k)) for k in bad if not torch.is_tensor(a[i].get(k)) or a[i][k].numel() == 1})


@pytest.mark.parametrize("mode", ["fused", "bridge"])
@pytest.mark.parametrize("kind", ["cluster", "cls", "vit", "desom"])
def test_stop_and_resume_in_a_fresh_model(kind, mode, tmp_path):
    """STOP steps, a checkpoint, a fresh model from the file, the remaining steps: every snapshot of steps STOP + 1..N (loss,
    logged terms, _it, iteration, opt._step, lr, temperature, gamma_t, BMUs) and the final parameters, gradients, moments and
    validation loss equal run A's.  The lr changes at steps 3 and 6; the resumed ViTSOM runs two steps host-driven and
    records its tape again, where run A replays."""
    c = R.case(kind)
    inputs = _inputs(kind, (c.batch,) * N)
    trace_a, final_a = _uninterrupted(kind, mode)
    lrs = [trace_a[i]["lr"] for i in range(1, N + 1)]
    if kind != "desom":                                              # (DESOM has no scheduler: desom.py:95-111)
        assert lrs[0] == lrs[2] != lrs[3] == lrs[5] != lrs[6] and lrs[6] != lrs[0], lrs
    model, opt, sched = R.fresh(c, DEV)
    trace_b = R.run_steps(model, opt, sched, inputs, 1, STOP, mode)
    path = R.save_snapshot(model, opt, sched, str(tmp_path / "stop.ckpt"))
    del model, opt, sched
    model, opt, sched = R.resume(c, path, DEV)
    assert model._it == trace_a[STOP]["_it"] and opt._step == STOP
    R.run_steps(model, opt, sched, inputs, STOP + 1, N, mode, trace_b)
    _no_differences(trace_a, trace_b, range(1, N + 1))
    bad = R.differences(final_a, R.final_state(model, inputs[0]))
    assert not bad, bad
    if kind in ("cluster", "cls"):
        ids_a, ids_b = ([t[i]["tape_id"] for i in range(1, N + 1)] for t in (trace_a, trace_b))
        assert ids_a[:2] == [0, 0] and ids_a[2] > 0 and ids_a[2:] == [ids_a[2]] * (N - 2), ids_a
        assert ids_b[:2] == [0, 0] and ids_b[2] == ids_b[3] > 0, ids_b
        assert ids_b[4:6] == [0, 0] and ids_b[6] == ids_b[7] > 0, ids_b


@pytest.mark.parametrize("kind,adamw_planes", [("cluster", False), ("planes", False), ("planes", True)])
def test_roll_back_a_live_model(kind, adamw_planes, tmp_path):
    """Five steps, so the tape is replaying; then the state taken after step 2 goes back into the SAME model, optimizer and
    scheduler and steps 3..5 run again: equal to the first pass.  The load writes the arena in place, so the tape stays
    valid and goes on replaying (asserted through its id); the prototypes' plane image is marked stale by the load and split
    again -- inside the tape with hooks.adamw_planes off, before it with the hook on.  The first step after the load also
    equals, BMUs included, that of a fresh model given the same file, which runs it host-driven."""
    from vit_som_amd import ops
    from vit_som_amd.tuning import hooks
    hooks.set(adamw_planes=adamw_planes)
    try:
        c = R.case(kind)
        inputs = _inputs(kind, (c.batch,) * 5)
        model, opt, sched = R.fresh(c, DEV)
        first = R.run_steps(model, opt, sched, inputs, 1, 2)
        path = R.save_snapshot(model, opt, sched, str(tmp_path / "after2.ckpt"))
        R.run_steps(model, opt, sched, inputs, 3, 5, trace=first)
        end_first = R.final_state(model)
        ids = [first[i]["tape_id"] for i in range(1, 6)]
        assert ids[:2] == [0, 0] and ids[2] == ids[3] == ids[4] > 0, ids
        som = model.som_layer
        image = som._wplanes
        if kind == "planes":
            assert som._planes_used and image is not None
            assert (som._wplanes_stamp == som._w_stamp()) == adamw_planes      # kept by the optimizer, or left behind by it

        R.resume(c, path, DEV, live=(model, opt, sched))
        assert model._it == first[2]["_it"] == int(model.iteration) and opt._step == 2
        assert opt.param_groups[0]["lr"] == first[2]["lr"] and sched.last_epoch == 0
        if kind == "planes":
            assert som._wplanes is image and som._wplanes_stamp != som._w_stamp()      # seen stale
        second = R.run_steps(model, opt, sched, inputs, 3, 5)
        _no_differences(first, second, range(3, 6))
        bad = R.differences(end_first, R.final_state(model))
        assert not bad, bad
        assert [second[i]["tape_id"] for i in range(3, 6)] == [ids[4]] * 3       # the same tape, still replaying
        if kind == "planes" and adamw_planes:
            split = ops.bmu_planes_alloc(*som.prototypes.shape, DEV)
            ops.bmu_planes_from(som.prototypes.detach(), split)
            assert som._wplanes_stamp == som._w_stamp() and torch.equal(split, som._wplanes)

        other, o3, s3 = R.resume(c, path, DEV)
        third = R.run_steps(other, o3, s3, inputs, 3, 3)
        assert third[3]["tape_id"] == 0
        assert torch.equal(third[3]["bmu"], second[3]["bmu"])
        _no_differences(second, third, [3])
    finally:
        hooks.reset()


@pytest.mark.parametrize("mode", ["fused", "bridge"])
@pytest.mark.parametrize("kind", ["cluster", "cls"])
def test_ragged_last_batch_between_replayed_steps(kind, mode):
    """B, B, B, B, B' < B, B, B: the epoch's short last batch gets a buffer set and a tape counter of its own between two
    replayed steps.  With the launch tape on and off: the same losses, logged terms, counters, parameters, gradients and
    moments; `iteration` advances once per step."""
    from vit_som_amd.tuning import hooks
    c = R.case(kind)
    B, short = c.batch, c.batch - 2
    sizes = (B, B, B, B, short, B, B)
    inputs = _inputs(kind, sizes)
    start = int(c.state["iteration"])

    def run(tape_on):
        hooks.set(launch_tape=tape_on)
        try:
            model, opt, sched = R.fresh(c, DEV)
            trace = R.run_steps(model, opt, sched, inputs, 1, len(sizes), mode)
            return trace, R.final_state(model)
        finally:
            hooks.reset()

    off, end_off = run(False)
    on, end_on = run(True)
    assert [off[i]["tape_id"] for i in range(1, 8)] == [0] * 7
    ids = [on[i]["tape_id"] for i in range(1, 8)]
    assert ids[:2] == [0, 0] and ids[2] > 0 and ids[4] == 0 and [ids[i] for i in (3, 5, 6)] == [ids[2]] * 3, ids
    for i in range(1, 8):
        assert on[i]["iteration"] == on[i]["_it"] == start + i and on[i]["bmu"].shape[0] == sizes[i - 1]
    _no_differences(off, on, range(1, 8))
    bad = R.differences(end_off, end_on)
    assert not bad, bad


@pytest.mark.parametrize("kind", ["cls", "cluster"])
def test_optimizer_state_against_torch_adamw(kind):
    """The state after three steps, edited as a foreign checkpoint would be (its own weight_decay per group, eps, lr), goes
    into FusedAdamW and into torch.optim.AdamW over clones of the parameters; both get the gradients of one
    train_step_fused and step once: p, exp_avg and exp_avg_sq agree per parameter by test_adamw_step's rule, and in
    classification mode neither touches the decoder.  Then weight_decay is edited in the live groups of both, and they step
    again: the kernel follows."""
    c = R.case(kind)
    inputs = _inputs(kind, (c.batch,) * 5)
    model, opt, sched = R.fresh(c, DEV)
    R.run_steps(model, opt, sched, inputs, 1, 3)
    sd = R.foreign_edit(opt.state_dict())
    opt.load_state_dict(sd)
    ref, names, leaves = R.torch_adamw_over(opt)
    ref.load_state_dict(sd)
    for g, rg, sg in zip(opt.param_groups, ref.param_groups, sd["param_groups"]):
        assert g["weight_decay"] == rg["weight_decay"] == sg["weight_decay"] and g["eps"] == rg["eps"] == 1e-6
        assert g["lr"] == rg["lr"] == 3e-3
    decoder = set(model._decoder_param_names()) if model.classification else set()
    assert bool(decoder) == (kind == "cls")
    a = model.arena

    def step_both(batch, count):
        model.train_step_fused(*(t.to(DEV) for t in batch))
        before = {n: a.p(n).detach().cpu().clone() for n in names}
        for n, leaf in zip(names, leaves):
            if n in decoder:
                assert not a.g(n).any(), n                                    # the same gradient for both: none
                leaf.grad = None
            else:
                leaf.grad = a.g(n).detach().cpu().clone()
        opt.step()
        ref.step()
        assert opt._step == count
        for n, leaf in zip(names, leaves):
            p, m, v = a.p(n), a.view(a.exp_avg, n), a.view(a.exp_avg_sq, n)
            st = ref.state[leaf]
            assert float(st["step"]) == (3 if n in decoder else count), n        # torch skips a parameter without a gradient
            assert R.adamw_close(p, leaf), (n, float((p.cpu() - leaf.detach()).abs().max()))
            assert R.adamw_close(m, st["exp_avg"]), (n, float((m.cpu() - st["exp_avg"]).abs().max()))
            assert R.adamw_close(v, st["exp_avg_sq"]), (n, float((v.cpu() - st["exp_avg_sq"]).abs().max()))
            if n in decoder:
                assert torch.equal(p.cpu(), before[n]) and torch.equal(leaf.detach(), before[n]), n
                assert not m.any() and not v.any(), n
            else:
                assert not torch.equal(leaf.detach(), before[n]), n

    step_both(inputs[3], 4)
    for i, (g, rg) in enumerate(zip(opt.param_groups, ref.param_groups)):
        g["weight_decay"] = rg["weight_decay"] = 0.5 - 0.03 * i
    step_both(inputs[4], 5)
