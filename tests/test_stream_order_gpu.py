"""The step's cross-stream ordering, checked from its recorded launches (tests/stream_order.py states the model).

Each case runs in a fresh child process with the recorder of test_step_trace_gpu.py on every library entry -- this time
keeping the pointer arguments -- from process start, for three steps: the window in which the pooled events are handed
out for the first time and in which a production run records its launch tape.  torch.cuda.synchronize is wrapped too:
one issued inside the window would be logged as a barrier (the step issues none).  The two device tables that name
operands (the LayerNorm job table, the transpose table) are read back when a call first names them or needs more rows of
them than were read -- the job table of a process's first step is rebuilt as it grows, and the allocator may hand the new
one the old address -- and once more after the run, where every table of the last step must still read the same: from
the second step on they are persistent.

Per case the parent asserts: no finding of the checker; the same wait resolution in every step; and, removing each
cross-stream wait of the middle step in turn, at least one load-bearing wait for every (recording stream -> waiting
stream) pair of the step -- removing all of them must produce races, or the check would be vacuous.

`python tests/test_stream_order_gpu.py --write` (re)writes tests/golden/step_access_trace.json, the same windows with
pointers as (buffer, offset); tests/test_stream_order_cpu.py runs the checker over it without a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]

import stream_order as so                                                   # noqa: E402
from test_step_trace_gpu import FIXTURE as LAUNCH_FIXTURE                   # noqa: E402
from test_step_trace_gpu import _build_case, _record, _stream_positions    # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "step_access_trace.json")
MARK = "STREAM-ORDER-JSON "
STEPS = 3
PLANES_B = 192                      # the smallest batch SOMLayer._planes_shape_ok accepts
# case -> (configuration of test_step_trace_gpu._build_case, hooks, what a step is, batch override)
CASES = {
    "host-vitsom_cluster_b96": ("vitsom_cluster_b96", {"launch_tape": False}, "train", None),
    "host-vitsom_ref_cls_tiny": ("vitsom_ref_cls_tiny", {"launch_tape": False}, "train", None),
    "host-vitcls_ref_hd8_pruned": ("vitcls_ref_hd8_pruned", {"launch_tape": False}, "train", None),
    "tape-vitsom_cluster_b96": ("vitsom_cluster_b96", {}, "train", None),               # hooks at their defaults: the third
    "tape-vitsom_ref_cls_tiny": ("vitsom_ref_cls_tiny", {}, "train", None),             # step is recorded, as in production
    "planes-train": ("vitsom_cluster_b96", {"launch_tape": False, "bmu_overlap": False}, "train", PLANES_B),
    "planes-bmu_overlap": ("vitsom_cluster_b96", {"launch_tape": False, "bmu_overlap": True}, "train", PLANES_B),
    "planes-forward": ("vitsom_cluster_b96", {"launch_tape": False}, "forward", PLANES_B),
    "exchange": ("vitsom_cluster_b96", {"launch_tape": False}, "exchange", None),
}


# ------------------------------------------------------------------------------------ child: record
def _device_words(address, nwords):
    """`nwords` 64-bit words of device memory at `address`, through the HIP runtime the process already holds."""
    path = "libamdhip64.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    host = (C.c_int64 * nwords)()
    rc = hip.hipMemcpy(host, C.c_void_p(address), 8 * nwords, 2)          # hipMemcpyDeviceToHost
    assert rc == 0, ("hipMemcpy", rc)
    return list(host)


def _child(case):
    sys.path[:0] = [ROOT, HERE]
    import torch
    from vit_som_amd import _lib, ops
    from vit_som_amd.tuning import hooks
    build, hook_values, kind, batch = CASES[case]
    log = []
    _record(_lib.lib, _lib.SIGNATURES, log)

    def allreduce(*args):               # logged on its stream and not run: nothing is reduced, an ordering check needs no values
        log.append(("vsom_comm_allreduce_sum", args))
        return 0
    _lib.lib.vsom_comm_allreduce_sum = allreduce
    tables = {}

    def with_table(name, where, nwords):
        inner = getattr(_lib.lib, name)             # the recording wrapper

        def rec(*args):
            rc = inner(*args)
            key, n = str(int(args[where])), nwords(args)
            if len(tables.get(key, ())) < n:        # first seen, or grown: one blocking copy, in a process's first step only
                tables[key] = _device_words(int(key), n)
            return rc
        setattr(_lib.lib, name, rec)
    with_table("vsom_layernorm_bwd_finish_many", 0, lambda a: (a[1] + a[2]) * 4)
    with_table("vsom_transpose_many", 2, lambda a: a[3] * 4)
    real_sync = torch.cuda.synchronize

    def sync(*a, **k):
        log.append(("barrier", ()))
        return real_sync(*a, **k)

    main = int(torch.cuda.current_stream().cuda_stream or 0)
    m, opt, x, y = _build_case(build)
    hooks.set(**hook_values)
    if batch is not None:
        x = torch.randn(batch, *x.shape[1:], generator=torch.Generator().manual_seed(5)).to(x.device)
        y = torch.zeros(batch, dtype=torch.int64, device=x.device)
    if kind == "exchange":              # two ranks and the library's communicator, set on the object: no process group is needed
        m.world_size, m._use_vsom_comm = 2, True

    def run_step():
        start = len(log)
        if kind == "forward":
            m._run_forward(x, need_decoder=False, fresh_w=True)
        else:
            m.train_step_fused(x, y)
            opt.step()
        return log[start:]

    torch.cuda.synchronize = sync
    steps = [run_step() for _ in range(STEPS)]
    torch.cuda.synchronize = real_sync
    res = {}
    if case.startswith("tape-"):
        replay = run_step()
        assert [n for n, _ in replay].count("vsom_tape_replay") == 3, [n for n, _ in replay]
        tape = m.vit._acts[x.shape[0]].tape
        res["tape_segment_ops"] = [ops.tape_segment_ops(tape.id, s) for s in range(4)]
        res["recorded_step"] = [i for i, s in enumerate(steps) if any(n == "vsom_tape_begin" for n, _ in s)]
    torch.cuda.synchronize()

    labels = {main: "main", int(m._side_stream.cuda_stream): "side"}
    if getattr(m, "_som_stream", None) is not None:
        labels[int(m._som_stream.cuda_stream)] = "som"
    if getattr(m, "_comm", None) is not None:
        labels[int(m._comm.cuda_stream)] = "comm"
    where = _stream_positions(_lib.SIGNATURES)
    out = []
    for step in steps:
        rows = []
        for name, args in step:
            if name == "barrier":
                rows.append([name, None, []])
                continue
            s = where[name]
            stream = None if s is None else labels.setdefault(int(args[s] or 0), "other%d" % len(labels))
            vals = [None if v is None else float(v) if isinstance(v, float) else int(v) if isinstance(v, int) else None
                    for i, v in enumerate(args) if i != s]
            rows.append([name, stream, vals])
        out.append(rows)
    for name, args in steps[-1]:                    # the tables the settled step uses have not changed since they were read
        key = {"vsom_layernorm_bwd_finish_many": 0, "vsom_transpose_many": 2}.get(name)
        if key is not None:
            key = str(int(args[key]))
            assert _device_words(int(key), len(tables[key])) == tables[key], (name, key)
    res["steps"] = out
    res["tables"] = tables
    print(MARK + json.dumps(res, separators=(",", ":")), flush=True)


# ------------------------------------------------------------------------------------ parent: check
def _header():
    with open(os.path.join(ROOT, "include", "vitsom_hip.h")) as f:
        return so.parse_header(f.read())


def _run(case):
    """-> (trace of the case's window, what else the child reported), each case under its own time limit."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=240)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(MARK)]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    got = json.loads(lines[0][len(MARK):])
    header = _header()
    calls = []
    for step, rows in enumerate(got.pop("steps")):
        for entry, stream, vals in rows:
            names = [n for n, kind in header.get(entry, ()) if kind != "stream"]
            assert len(names) == len(vals), (entry, names, vals)
            calls.append(so.call(entry, stream, step, **dict(zip(names, vals))))
    return so.make_trace(calls, got.pop("tables")), got


def _summary(case, trace, report):
    launches = sum(1 for c in trace["calls"] if c["stream"] is not None and c["entry"] not in (so.RECORD, so.WAIT))
    pairs = ", ".join("%s->%s %d/%d" % (a, b, n[1], n[0]) for (a, b), n in sorted(report["pairs"].items()))
    return ("%s: %d calls checked (%d launches), %d conflicting-range pairs examined, %d cross-stream waits in the middle step, "
            "%d load-bearing [%s], %d races with every wait removed"
            % (case, len(trace["calls"]), launches, report["conflict_pairs"], report["waits"], report["load_bearing"], pairs,
               report["all_removed_races"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_step_is_ordered(case):
    trace, extra = _run(case)
    assert not any(c["entry"] == so.BARRIER for c in trace["calls"]), "the step synchronises with the host"
    findings = so.check(trace)
    for f in findings[:20]:
        print(f["text"])
    assert not findings, "%d findings, the first: %s" % (len(findings), findings[0]["text"])
    res = so.resolution_by_step(trace)
    assert sorted(res) == list(range(STEPS))
    for step in range(STEPS - 1):
        assert res[step] == res[STEPS - 1], (step, so.describe_resolution(trace, step), so.describe_resolution(trace, STEPS - 1))
    report = so.mutation_report(trace, 1)
    print(_summary(case, trace, report))
    assert report["waits"] > 0 and report["all_removed_races"] > 0
    idle = [k for k, n in report["pairs"].items() if n[1] == 0]
    assert not idle, "no wait of these (recording, waiting) stream pairs is load-bearing: %s" % idle
    if case.startswith("tape-"):
        with open(LAUNCH_FIXTURE) as f:
            ref = json.load(f)[case[len("tape-"):]]
        assert extra["recorded_step"] == [STEPS - 1]                       # the third step is the one the tape holds
        assert extra["tape_segment_ops"] == ref["tape_segment_ops"]


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        _child(sys.argv[2])
    elif sys.argv[1:2] == ["--write"]:
        out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        header = _header()
        with open(out, "w") as f:
            json.dump(so.encode_fixture({c: _run(c)[0] for c in CASES}, header), f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {out} ({os.path.getsize(out)} bytes)")
    else:
        raise SystemExit("usage: test_stream_order_gpu.py --write [FILE]")
