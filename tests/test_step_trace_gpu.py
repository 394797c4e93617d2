"""The launch sequence of the fused training step, call by call, against tests/golden/step_launch_trace.json.

Every entry of _lib.SIGNATURES is wrapped on the loaded library object with a recorder, in a fresh child process per
case (library event ids start from zero there).  The step then runs host-driven (hooks.launch_tape = False) with its
optimizer step, for at least four steps and until the pooled events have wrapped once, and -- the ViTSOM cases --
through the launch tape: two host-driven steps, the recorded one, two replays, plus ops.tape_segment_ops of the four
segments.  A call is written "entry|stream|arguments": the stream argument (the one include/vitsom_hip.h declares
vsom_stream_t) relabelled main / side / som / other<k> by comparing handles, and every argument whose declared type
is not a pointer -- for vsom_event_record / vsom_stream_wait_event that is the event id.  Pointers are left out: they
differ from process to process.

The fixture holds, per case, the table of distinct calls and each step as indices into it; nothing in it is typed by
hand.  `python tests/test_step_trace_gpu.py --write` (re)writes it and uses no name younger than the fixture, so it
runs on the commit whose launch order is the yardstick."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "step_launch_trace.json")
CASES = ["vitsom_cluster_b96", "vitsom_ref_cls_tiny", "vitcls_ref_hd8_pruned"]
MIN_STEPS, MAX_STEPS = 4, 64
MARK = "STEP-TRACE-JSON "


# ------------------------------------------------------------------------------------ child: record
def _stream_positions(names):
    """entry -> index of its vsom_stream_t argument (None when it has none), from the C header."""
    with open(os.path.join(ROOT, "include", "vitsom_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")
        out[name] = next((i for i, a in enumerate(args) if a.strip().startswith("vsom_stream_t")), None)
    return out


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)


def _record(lib, signatures, log):
    for name in signatures:
        def rec(*args, _fn=getattr(lib, name), _name=name):
            log.append((_name, args))
            return _fn(*args)
        setattr(lib, name, rec)


def _build_case(case):
    """-> (model, optimizer, x, y) as the suite's own tests of these configurations build them."""
    import copy
    import numpy as np
    import torch
    import vit_som_amd
    from vit_som_amd.tuning import hooks
    dev = "cuda:0"
    if case == "vitsom_cluster_b96":                     # test_model_gpu._run_switch_combinations
        from oracle.gen_golden import make_config
        cfg = make_config(3, 32, 4, 192, 4, 3, 96, 2, (12, 12), 0, 96)
        torch.manual_seed(0)
        m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=dev)
        m.set_schedule(5000, 500)
        m._it = 100
        x = torch.randn(96, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev)
        y = torch.zeros(96, dtype=torch.int64, device=dev)
    elif case == "vitsom_ref_cls_tiny":
        z = np.load(os.path.join(HERE, "golden", "ref_cls_tiny.npz"), allow_pickle=False)
        m = vit_som_amd.ViTSOM(json.loads(str(z["config_json"])), device=dev)
        m.load_state_dict({k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")})
        m.set_schedule(int(z["n_train"]), int(z["est_steps"]))
        x, y = torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["y"]).to(dev)
    else:
        hooks.set(cls_prune=True)
        z = np.load(os.path.join(HERE, "golden", "ref_vitcls_hd8.npz"), allow_pickle=False)
        m = vit_som_amd.ViTClassifier(json.loads(str(z["config"])), device=dev)
        m.load_state_dict({k: torch.from_numpy(z["param/" + k]) for k in (str(s) for s in z["state_keys"])})
        x, y = torch.from_numpy(z["x0"]).to(dev), torch.from_numpy(z["y0"]).to(dev)
    (opt,), _ = m.configure_optimizers()
    return m, opt, x, y


def _child(case):
    sys.path[:0] = [ROOT, HERE]
    import torch
    from vit_som_amd import _lib, ops
    from vit_som_amd.tuning import hooks
    log = []
    _record(_lib.lib, _lib.SIGNATURES, log)
    main = int(torch.cuda.current_stream().cuda_stream or 0)
    m, opt, x, y = _build_case(case)

    def run_step():
        start = len(log)
        m.train_step_fused(x, y)
        opt.step()
        return log[start:]

    hooks.set(launch_tape=False)
    host, full_at = [], None
    while len(host) < MAX_STEPS:
        host.append(run_step())
        if full_at is None and len(_lib.Event._pool) == _lib.Event.POOL:
            full_at = len(host)                          # the pool filled during this step: the next one runs wrapped
        if len(host) >= MIN_STEPS and full_at is not None and len(host) > full_at:
            break
    taped, segments = [], None
    if hasattr(m, "som_layer"):                          # the launch tape is ViTSOM's; ViTClassifier is host-driven only
        hooks.set(launch_tape=True)
        taped = [run_step() for _ in range(5)]
        tape = m.vit._acts[x.shape[0]].tape
        segments = [ops.tape_segment_ops(tape.id, s) for s in range(4)]
    torch.cuda.synchronize()

    labels = {main: "main", int(m._side_stream.cuda_stream): "side", int(m._som_stream.cuda_stream): "som"}
    where = _stream_positions(_lib.SIGNATURES)
    table, index = [], {}

    def encode(step):
        out = []
        for name, args in step:
            argtypes, s = _lib.SIGNATURES[name][1], where[name]
            stream = "-" if s is None else labels.setdefault(int(args[s] or 0), "other%d" % (len(labels) - 3))
            vals = [repr(float(v)) if t in (C.c_float, C.c_double) else str(int(v))
                    for i, (t, v) in enumerate(zip(argtypes, args)) if i != s and not _is_pointer(t)]
            call = "|".join([name, stream, ",".join(vals)])
            if call not in index:
                index[call] = len(table)
                table.append(call)
            out.append(index[call])
        return out

    res = {"host_steps": [encode(s) for s in host], "taped_steps": [encode(s) for s in taped], "tape_segment_ops": segments,
           "pool_wrapped_after_step": full_at, "calls": table}
    print(MARK + json.dumps(res, separators=(",", ":")), flush=True)


# ------------------------------------------------------------------------------------ parent: compare
def _trace(case):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(MARK)]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0][len(MARK):])


def _first_difference(got, ref):
    for key in ("host_steps", "taped_steps"):
        a, b = [[got["calls"][i] for i in s] for s in got[key]], [[ref["calls"][i] for i in s] for s in ref[key]]
        for n, (sa, sb) in enumerate(zip(a, b)):
            for k, (ca, cb) in enumerate(zip(sa, sb)):
                if ca != cb:
                    return f"{key}[{n}] call {k}: got {ca!r}, fixture {cb!r}"
            if len(sa) != len(sb):
                return f"{key}[{n}]: got {len(sa)} calls, fixture {len(sb)}; first extra {(sa + sb)[min(len(sa), len(sb))]!r}"
        if len(a) != len(b):
            return f"{key}: got {len(a)} steps, fixture {len(b)}"
    for key in ("tape_segment_ops", "pool_wrapped_after_step"):
        if got[key] != ref[key]:
            return f"{key}: got {got[key]}, fixture {ref[key]}"
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_step_launch_trace_matches_fixture(case):
    with open(FIXTURE) as f:
        ref = json.load(f)[case]
    got = _trace(case)
    assert len(got["host_steps"]) >= MIN_STEPS and got["pool_wrapped_after_step"] is not None
    assert len(got["host_steps"]) > got["pool_wrapped_after_step"]       # a whole step ran on the wrapped pool
    diff = _first_difference(got, ref)
    if diff is not None:
        print(diff)
    assert diff is None, diff
    assert got == ref


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        _child(sys.argv[2])
    elif sys.argv[1:2] == ["--write"]:
        out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        with open(out, "w") as f:
            json.dump({c: _trace(c) for c in CASES}, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {out} ({os.path.getsize(out)} bytes)")
    else:
        raise SystemExit("usage: test_step_trace_gpu.py --write [FILE]")
