"""tests/stream_order.py on hand-written traces, Event.pooled(), and the two committed traces of the step.  No GPU."""
import json
import os
import subprocess
import sys

import pytest

import stream_order as so
from stream_order import call

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "vitsom_hip.h")) as f:
        return so.parse_header(f.read())


# ------------------------------------------------------------------------------------ hand-written traces
BUF, OTHER = 0x10000, 0x90000          # two allocations, far apart
N = 256                                # floats per operand


def fill(stream, p=BUF, n=N, at=0):
    return call("vsom_fill", stream, at, p=p, n=n, value=0.0)


def scale(stream, p=BUF, n=N, by=OTHER, at=0):
    """Reads and writes p[0:n], reads one float at `by`."""
    return call("vsom_scale_by", stream, at, p=p, n=n, scale_dev=by)


def reads(stream, p=BUF, n=N, at=0):
    """A call that only reads p[0:n] (as the scale of a scale_by over another allocation)."""
    assert n == 1
    return call("vsom_scale_by", stream, at, p={"main": 0x500000, "side": 0x600000}[stream], n=1, scale_dev=p)


def record(ev, stream, at=0):
    return call(so.RECORD, stream, at, ev=ev)


def wait(stream, ev, at=0):
    return call(so.WAIT, stream, at, ev=ev)


def fork_join(with_wait=True, rerecord=None):
    """main writes BUF, side scales it (a read-write) behind an event, main reads it back behind a second event."""
    calls = [fill("main"), record(7, "main")]
    if rerecord:
        calls.append(record(7, rerecord))
    if with_wait:
        calls.append(wait("side", 7))
    calls += [scale("side"), record(8, "side"), wait("main", 8), scale("main")]
    return so.make_trace(calls)


def test_header_names_every_entry_of_the_access_table(header):
    assert not [e for e in so.ACCESS if e not in header]
    assert header["vsom_stream_wait_event"] == [("stream", "stream"), ("ev", "val")]
    assert ("ws", "ptr") in header["vsom_linear_bwd_weight"] and ("ws_bytes", "val") in header["vsom_linear_bwd_weight"]


def test_correct_fork_and_join_is_clean():
    assert so.check(fork_join()) == []


def test_missing_wait_is_a_raw_race_between_the_right_calls():
    trace = fork_join(with_wait=False)
    found = so.check(trace)
    assert found and all(f["type"] == "race" for f in found)
    f = found[0]
    first, second = trace["calls"][f["first"]], trace["calls"][f["second"]]
    assert (f["kind"], first["entry"], first["stream"], first["pos"]) == ("RAW", "vsom_fill", "main", 0)
    assert (second["entry"], second["stream"], second["pos"]) == ("vsom_scale_by", "side", 2)
    assert (f["first_arg"], f["second_arg"], f["buffer"], f["range"]) == ("p", "p", -1, (BUF, BUF + 4 * N))
    assert "step 0 #0 vsom_fill on main" in f["text"] and "step 0 #2 vsom_scale_by on side" in f["text"]
    assert len(found) == 1                      # the join back to main is intact: nothing else is unordered


def test_event_rerecorded_on_another_stream_before_the_wait_is_flagged():
    trace = fork_join(rerecord="som")
    found = so.check(trace)
    assert [f["kind"] for f in found] == ["RAW"]           # the wait now sees som's record: main's fill is not ordered before
    assert trace["calls"][found[0]["first"]]["entry"] == "vsom_fill"
    res = so.wait_resolution(trace)
    assert (res[0]["stream"], res[0]["record_stream"], trace["calls"][res[0]["record"]]["pos"]) == ("side", "som", 2)
    # ... and re-recorded on the waiting stream itself it is a wait that orders nothing
    found = so.check(fork_join(rerecord="side"))
    assert sorted(f["type"] for f in found) == ["race", "self-wait"]


def test_war_and_waw():
    war = so.make_trace([reads("side", n=1), fill("main", n=1)])
    waw = so.make_trace([fill("side"), fill("main")])
    raw = so.make_trace([fill("side", n=1), reads("main", n=1)])
    assert [(f["kind"], f["first_arg"], f["second_arg"]) for f in so.check(war)] == [("WAR", "scale_dev", "p")]
    assert [f["kind"] for f in so.check(waw)] == ["WAW"]
    assert [f["kind"] for f in so.check(raw)] == ["RAW"]
    for t in (war, waw, raw):                   # the same pairs, ordered through an event
        a, b = t["calls"]
        assert so.check(so.make_trace([a, record(1, a["stream"]), wait(b["stream"], 1), b])) == []
    # two reads never conflict; one stream never races with itself
    assert so.check(so.make_trace([reads("side", n=1), reads("main", n=1)])) == []
    assert so.check(so.make_trace([fill("main"), scale("main"), fill("main")])) == []


def test_ranges_that_touch_are_clean_and_one_byte_of_overlap_is_a_race():
    assert so.check(so.make_trace([fill("main", BUF, N), fill("side", BUF + 4 * N, N)])) == []
    # a strided operand: rows of 3 floats every 8 -> the hull ends 3 floats into the last row
    rows = call("vsom_rows_add", "side", 0, src=OTHER, lds=8, dst=BUF, ldd=8, rows=4, cols=3)
    end = BUF + ((4 - 1) * 8 + 3) * 4
    assert so.check(so.make_trace([rows, fill("main", end, N)])) == []
    found = so.check(so.make_trace([rows, fill("main", end - 4, N)]))
    assert [(f["kind"], f["range"]) for f in found] == [("WAW", (end - 4, end))]
    # overlap of exactly one byte: a one-byte workspace against the float in front of it
    one = call("vsom_cross_entropy_ls", "side", 0, logits=None, y=None, smoothing=0.0, loss_sum=None, dlogits=None, grad_scale=0.0,
               B=1, C=1, ws=BUF + 4 * N - 1, ws_bytes=1)
    found = so.check(so.make_trace([fill("main", BUF, N), one]))
    assert [(f["kind"], f["second_arg"], f["range"]) for f in found] == [("RAW", "ws", (BUF + 4 * N - 1, BUF + 4 * N))]
    one["args"]["ws"] += 1
    assert so.check(so.make_trace([fill("main", BUF, N), one])) == []


def test_wait_before_any_record_is_reported():
    trace = so.make_trace([wait("side", 3), fill("side"), record(3, "main")])
    found = so.check(trace)
    assert [f["type"] for f in found] == ["unrecorded-wait"] and found[0]["second"] == 0
    assert so.wait_resolution(trace)[0]["record"] is None


def test_deferred_join_resolves_to_the_record_it_names():
    """Block j's side work is joined two blocks later: with an event per record the wait finds its own record, with one
    shared id it finds the latest."""
    def blocks(ids):
        calls, pending = [], []
        for j, ev in enumerate(ids):
            if len(pending) > 1:
                calls.append(wait("main", pending.pop(0)))
            calls += [fill("main", BUF + 0x1000 * j), scale("side", OTHER + 0x1000 * j, by=0x700000), record(ev, "side")]
            pending.append(ev)
        return so.make_trace(calls)
    distinct, shared = blocks([1, 2, 3, 4]), blocks([0, 0, 0, 0])
    pos = lambda t: [(t["calls"][r["wait"]]["pos"], t["calls"][r["record"]]["pos"]) for r in so.wait_resolution(t)]   # noqa: E731
    assert pos(distinct) == [(6, 2), (10, 5)]              # two records back
    assert pos(shared) == [(6, 5), (10, 9)]                # the previous block's: what Event.pooled() used to give
    # names, not numbers: any other distinct ids resolve alike
    assert pos(blocks([40, 9, 191, 0])) == pos(distinct)
    assert so.resolution_by_step(distinct) == so.resolution_by_step(blocks([40, 9, 191, 0]))


def test_barrier_orders_everything_and_missing_rows_are_named():
    racy = [fill("side"), fill("main")]
    assert so.check(so.make_trace(racy)) != []
    assert so.check(so.make_trace([racy[0], call(so.BARRIER), racy[1]])) == []
    with pytest.raises(so.Incomplete, match="vsom_reduce_slabs"):
        so.check(so.make_trace([call("vsom_reduce_slabs", "main", 0, slabs=BUF, stride=4, nslabs=2, out=OTHER, n=4)]))
    # an entry without a stream argument launches nothing and needs no row
    assert so.check(so.make_trace([call("vsom_get_gemm_mode")])) == []
    with pytest.raises(so.Incomplete, match="table"):
        so.check(so.make_trace([call("vsom_layernorm_bwd_finish_many", "main", 0, jobs_dev=BUF, first=0, count=1, max_cols=8)]))


def test_table_driven_entries_take_their_ranges_from_the_table():
    part, dgamma, dbeta, cols, nblk = 0x200000, 0x300000, 0x300100, 8, 2
    jobs = {so.ptr_key(BUF): [0, 0, 0, 0, part, dgamma, dbeta, (nblk << 32) | cols]}
    finish = call("vsom_layernorm_bwd_finish_many", "main", 0, jobs_dev=BUF, first=1, count=1, max_cols=cols)
    acc = {(name, mode, lo, hi) for _, name, mode, _, lo, hi in so.accesses(so.make_trace([finish], jobs))}
    assert acc == {("jobs_dev", "r", BUF + 32, BUF + 64), ("jobs_dev.part", "r", part, part + nblk * 8 * cols),
                   ("jobs_dev.dgamma", "w", dgamma, dgamma + 4 * cols), ("jobs_dev.dbeta", "w", dbeta, dbeta + 4 * cols)}
    found = so.check(so.make_trace([fill("side", dbeta, cols), finish], jobs))
    assert [(f["kind"], f["second_arg"]) for f in found] == [("WAW", "jobs_dev.dbeta")]
    table = {so.ptr_key(BUF): [0, 64, 2, 3, 6, 0, 3, 2]}           # {src_off, dst_off, rows, cols} in floats
    tr = call("vsom_transpose_many", "main", 0, src_base=0x400000, dst_base=0x500000, table=BUF, count=2, max_rows=3, max_cols=3)
    acc = {(name, mode, lo, hi) for _, name, mode, _, lo, hi in so.accesses(so.make_trace([tr], table))}
    assert acc == {("table", "r", BUF, BUF + 64), ("src_base", "r", 0x400000, 0x400000 + 24), ("dst_base", "w", 0x500000 + 256, 0x500000 + 280),
                   ("src_base", "r", 0x400000 + 24, 0x400000 + 48), ("dst_base", "w", 0x500000, 0x500000 + 24)}


def test_mutation_report_counts_load_bearing_waits():
    trace = fork_join()
    rep = so.mutation_report(trace, 0)
    assert (rep["waits"], rep["load_bearing"], rep["pairs"]) == (2, 2, {("main", "side"): [1, 1], ("side", "main"): [1, 1]})
    assert rep["all_removed_races"] > 0
    # a wait that duplicates an edge the trace already has is not load-bearing
    calls = [dict(c) for c in trace["calls"]]
    calls[3:3] = [record(9, "main"), wait("side", 9)]
    rep = so.mutation_report(so.make_trace(calls), 0)
    assert (rep["waits"], rep["load_bearing"]) == (3, 1)    # either of the two main -> side waits alone still orders the fill


# ------------------------------------------------------------------------------------ Event.pooled()
POOLED_CHILD = r"""
import json, sys
from vit_som_amd._lib import Event
POOL = Event.POOL
ids = [Event.pooled().id for _ in range(3 * POOL)]
print("POOLED " + json.dumps({"pool": POOL, "ids": ids, "events": Event._next_id}))
"""


@pytest.fixture(scope="module")
def pooled():
    """3 * POOL consecutive Event.pooled() ids of a fresh process (ids are process-wide and capped at 512; Event() touches
    no device)."""
    p = subprocess.run([sys.executable, "-c", POOLED_CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("POOLED ")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0][len("POOLED "):])


def test_pooled_events_are_round_robin_from_the_first_call(pooled):
    POOL, ids = pooled["pool"], pooled["ids"]
    assert len(ids) == 3 * POOL and pooled["events"] == POOL            # the pool never grows past POOL events
    bad = [k for k in range(2 * POOL + 1) if len(set(ids[k:k + POOL])) != POOL]
    assert not bad, "windows of %d pooled ids with a repeat start at calls %s ...; the first ids are %s" % (POOL, bad[:5], ids[:8])
    assert ids[POOL:2 * POOL] == ids[:POOL] == ids[2 * POOL:]


def test_record_deferred_past_a_pool_of_calls_resolves_to_itself(pooled):
    """A record on the side stream, POOL - 1 further pooled records on main, then the wait: it must find its own record --
    from the first call of a process (the pool filling), in the middle of the fill and after the wrap."""
    POOL, ids = pooled["pool"], pooled["ids"]
    for start in (0, POOL // 2, POOL + 5, 2 * POOL):
        calls = [record(ids[start], "side")] + [record(e, "main") for e in ids[start + 1:start + POOL]] + [wait("main", ids[start])]
        res = so.wait_resolution(so.make_trace(calls))
        assert (res[0]["record"], res[0]["record_stream"]) == (0, "side"), (start, res)


# ------------------------------------------------------------------------------------ the committed traces
def _launch_cases():
    with open(os.path.join(HERE, "golden", "step_launch_trace.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", ["vitsom_cluster_b96", "vitsom_ref_cls_tiny", "vitcls_ref_hd8_pruned"])
def test_launch_fixture_resolves_every_step_like_the_wrapped_one(header, case):
    """Each host step of step_launch_trace.json -- the first ones run while the pool fills -- and the host-visible taped
    steps (two host-driven, then the recorded one) must resolve their waits as the last, wrapped host step does."""
    ref = _launch_cases()[case]
    trace = so.from_launch_fixture(ref, header)
    res = so.resolution_by_step(trace)
    n_host = len(ref["host_steps"])
    last = n_host - 1
    assert ref["pool_wrapped_after_step"] is not None and last >= ref["pool_wrapped_after_step"]
    steps = list(range(n_host)) + [n_host + k for k, s in enumerate(ref["taped_steps"][:3])]
    assert res[last] and all(s in res for s in steps)
    wrong = []
    for s in steps:
        ours, theirs = so.describe_resolution(trace, s), so.describe_resolution(trace, last)
        assert len(ours) == len(theirs), (s, len(ours), len(theirs))
        wrong += ["step %d: %s; the wrapped step %d: %s" % (s, a, last, b)
                  for a, b, ra, rb in zip(ours, theirs, res[s], res[last]) if ra != rb]
    assert not wrong, "%d waits resolve differently:\n%s" % (len(wrong), "\n".join(wrong[:12]))
    assert not [f for f in so._clocks(trace)[1] if f[1] is None]        # every wait finds a record


def _access_cases():
    with open(os.path.join(HERE, "golden", "step_access_trace.json")) as f:
        return json.load(f)


ACCESS_CASES = ["host-vitsom_cluster_b96", "host-vitsom_ref_cls_tiny", "host-vitcls_ref_hd8_pruned", "tape-vitsom_cluster_b96",
                "tape-vitsom_ref_cls_tiny", "planes-train", "planes-bmu_overlap", "planes-forward", "exchange"]


def test_access_fixture_holds_every_case():
    assert sorted(_access_cases()["cases"]) == sorted(ACCESS_CASES)


@pytest.mark.parametrize("case", ACCESS_CASES)
def test_access_fixture_is_clean(header, case):
    trace = so.decode_fixture(_access_cases(), case, header)
    launches = [c for c in trace["calls"] if c["stream"] is not None]
    assert len(launches) > 50 and len({c["stream"] for c in launches}) >= 2
    found = so.check(trace)
    assert not found, "%d findings, the first: %s" % (len(found), found[0]["text"])
    res = so.resolution_by_step(trace)
    assert len(res) == 3 and res[0] == res[1] == res[2]
    rep = so.mutation_report(trace, 1)
    assert rep["all_removed_races"] > 0 and rep["load_bearing"] > 0
    assert not [k for k, n in rep["pairs"].items() if n[1] == 0], rep["pairs"]
