"""A happens-before checker for the training step's recorded library calls.  Pure Python: no GPU, no library.

A *trace* is {"calls": [...], "tables": {...}}: the library calls of one or more consecutive steps in the order the host
issued them, each a dict {"step", "pos", "entry", "stream", "args"} -- `stream` the label of the call's vsom_stream_t
argument (None when the entry has none), `args` the other arguments by the names include/vitsom_hip.h gives them, by-value
arguments as numbers and pointers as `ptr` values: None (NULL), an integer address, or (buffer, byte offset).  `tables`
maps the pointer of a device table (ptr_key) to its 64-bit words, for the two entries whose operands are named by a table
in device memory.  A call {"entry": "barrier"} stands for a host synchronisation the recorder saw.

Ordering model (HIP's):
  * calls on one stream are ordered by issue;
  * vsom_event_record(ev, s) snapshots everything issued on s so far (and everything s was already ordered after);
  * vsom_stream_wait_event(s, ev) orders everything issued LATER on s after the snapshot ev holds at the moment of the
    wait call: host issue order decides which record a wait sees.  An event id is a name and nothing else;
  * a wait on an event that was never recorded orders nothing (HIP treats it as complete) and is reported;
  * NO implicit ordering between the default stream and the others (torch creates its side streams non-blocking), and no
    host synchronisation inside or between steps unless the trace holds a barrier.
One vector clock per stream implements this: a call's clock says, per stream, how many of that stream's calls are ordered
before it.  Call A on stream a happens before call B iff B's clock for a has reached A's own count.

ACCESS gives, per C entry point, the byte ranges a call reads and writes.  It is written out from include/vitsom_hip.h
(const pointer = read, non-const = write or read-write, extents from the documented shapes, ws / part with their *_bytes
argument) and NOT derived from the kernels.  A strided operand is the hull ((rows - 1) * ld + cols) * 4 bytes.  Every entry
of a checked trace that has a stream argument must have a row: there is no skip list and no list of excused races.
Refinements of a hull to an exact row set (base, row bytes, stride, rows): none -- no hull reported a conflict that the
exact sets do not have.

Findings: "race" (two calls on different streams, overlapping ranges, at least one writing, the earlier not ordered before
the later; kind RAW / WAR / WAW by what the earlier and the later call do), "unrecorded-wait" and "self-wait" (a wait
that resolves to a record made on the waiting stream itself: it orders nothing the stream's own order does not).

Not covered: torch's own kernels (copy_, fill_, zero_, allocations) are invisible to the recorder.  They run on torch's
current stream, the main stream of the step, so a cross-stream hazard through such an op is not seen.  Replayed tape
segments are not visible call by call either; the recorded step is what a tape holds."""
import bisect
import re

F = 4          # bytes per float
RECORD, WAIT, BARRIER = "vsom_event_record", "vsom_stream_wait_event", "barrier"


# ------------------------------------------------------------------------------------ the C header
def parse_header(text):
    """entry -> [(argument name, kind)], kind in "ptr" / "stream" / "val", for every prototype of the header."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, arglist in re.findall(r"\b(vsom_\w+)\s*\(([^)]*)\)\s*;", text):
        args = []
        for a in (s.strip() for s in arglist.split(",")):
            if a in ("", "void"):
                continue
            kind = "stream" if a.startswith("vsom_stream_t") else "ptr" if "*" in a else "val"
            args.append((re.search(r"(\w+)\s*$", a).group(1), kind))
        out[name] = args
    return out


# ------------------------------------------------------------------------------------ pointers
def ptr(v):
    """Normal form of a pointer argument: None, or (buffer, byte offset) with buffer -1 for a raw address."""
    if v is None or v == 0:
        return None
    if isinstance(v, int):
        return (-1, v)
    return (int(v[0]), int(v[1]))


def ptr_key(v):
    """The key of a pointer in trace["tables"] (and its text in the fixture): "0", "<address>" or "b<buffer>+<offset>"."""
    p = ptr(v)
    return "0" if p is None else str(p[1]) if p[0] < 0 else "b%d+%d" % p


def ptr_from_key(s):
    if isinstance(s, str) and s.startswith("b"):
        b, off = s[1:].split("+")
        return (int(b), int(off))
    return ptr(int(s))


# ------------------------------------------------------------------------------------ access table
def _hull(rows, ld, cols):
    return ((rows - 1) * ld + cols) * F if rows > 0 else 0


def _linear_common(a):
    M, N, K = a["M"], a["N"], a["K"]
    return [("X", "r", _hull(M, a["ldx"], K)), ("W", "r", N * K * F), ("bias", "r", N * F)], M, N, K


def _linear_fwd(a, t):
    acc, M, N, K = _linear_common(a)
    return acc + [("Y", "w", _hull(M, a["ldy"], N))]


def _linear_act_fwd(a, t):
    acc, M, N, K = _linear_common(a)
    return acc + [("Ygrad", "w", M * N * F), ("Yact", "w", M * N * F)]


def _linear_residual_fwd(a, t):
    acc, M, N, K = _linear_common(a)
    return acc + [("R", "r", _hull(min(M, a["r_mod"]), a["ldr"], N)), ("Y", "w", _hull(M, a["ldy"], N))]


def _linear_bwd_input(wname):
    def row(a, t):
        M, N, K = a["M"], a["N"], a["K"]
        return [("dY", "r", _hull(M, a["lddy"], N)), (wname, "r", N * K * F), ("gelu_grad", "r", M * K * F),
                ("dX", "rw" if a["accumulate"] else "w", _hull(M, a["lddx"], K))]
    return row


def _transpose_many(a, t):
    out = [("table", "r", a["count"] * 32)]
    words = t(a["table"], a["count"] * 4)
    for i in range(a["count"]):
        src_off, dst_off, rows, cols = words[4 * i:4 * i + 4]
        out += [("src_base", "r", rows * cols * F, src_off * F), ("dst_base", "w", rows * cols * F, dst_off * F)]
    return out


def _linear_bwd_weight(a, t):
    M, N, K = a["M"], a["N"], a["K"]
    return [("dY", "r", _hull(M, a["lddy"], N)), ("X", "r", _hull(M, a["ldx"], K)), ("dW", "w", N * K * F), ("db", "w", N * F),
            ("ws", "rw", a["ws_bytes"])]


def _patch(a):
    n = (a["S"] // a["p"]) ** 2
    return n, a["C"] * a["p"] * a["p"]


def _patch_embed_fwd(a, t):
    (n, pd), B, E = _patch(a), a["B"], a["E"]
    return [("img", "r", B * a["C"] * a["S"] * a["S"] * F), ("Wpe", "r", E * pd * F), ("bpe", "r", E * F), ("pos", "r", (n + 1) * E * F),
            ("cls_token", "r", E * F), ("tokens", "w", B * (n + 1) * E * F), ("xp_ws", "w", B * n * pd * F)]


def _patch_embed_bwd(a, t):
    (n, pd), B, E = _patch(a), a["B"], a["E"]
    return [("dtokens", "r", B * (n + 1) * E * F), ("xp_ws", "r", B * n * pd * F), ("dWpe", "w", E * pd * F), ("dbpe", "w", E * F),
            ("dcls_token", "w", E * F), ("ws", "rw", a["ws_bytes"])]


def _layernorm_fwd(a, t):
    r, c = a["rows"], a["cols"]
    return [("X", "r", r * c * F), ("gamma", "r", c * F), ("beta", "r", c * F), ("Y", "w", r * c * F), ("mean", "w", r * F),
            ("rstd", "w", r * F)]


def _ln_bwd_reads(r, c):
    return [("dY", "r", r * c * F), ("X", "r", r * c * F), ("mean", "r", r * F), ("rstd", "r", r * F), ("gamma", "r", c * F),
            ("resid", "r", r * c * F), ("dX", "w", r * c * F)]


def _layernorm_bwd(a, t):
    r, c = a["rows"], a["cols"]
    return _ln_bwd_reads(r, c) + [("dgamma", "w", c * F), ("dbeta", "w", c * F), ("ws", "rw", a["ws_bytes"])]


def _layernorm_bwd_partial(a, t):
    return _ln_bwd_reads(a["rows"], a["cols"]) + [("part", "w", a["part_bytes"])]


def _layernorm_bwd_finish_many(a, t):
    first, count = a["first"], a["count"]
    out = [("jobs_dev", "r", count * 32, first * 32)]
    words = t(a["jobs_dev"], (first + count) * 4)
    for j in range(first, first + count):
        part, dgamma, dbeta, shape = words[4 * j:4 * j + 4]
        nblk, cols = int(shape) >> 32, int(shape) & 0xFFFFFFFF
        out += [("jobs_dev.part", "r", nblk * 8 * cols, 0, part), ("jobs_dev.dgamma", "w", cols * F, 0, dgamma),
                ("jobs_dev.dbeta", "w", cols * F, 0, dbeta)]
    return out


def _ln_fused_reads(a):
    M, N, K = a["M"], a["N"], a["K"]
    return [("dY", "r", _hull(M, a["lddy"], N)), ("Wt", "r", K * N * F), ("X", "r", M * K * F), ("mean", "r", M * F), ("rstd", "r", M * F),
            ("gamma", "r", K * F), ("resid", "r", M * K * F), ("dX", "w", M * K * F)]


def _linear_bwd_input_ln(a, t):
    return _ln_fused_reads(a) + [("dgamma", "w", a["K"] * F), ("dbeta", "w", a["K"] * F), ("ws", "rw", a["ws_bytes"])]


def _linear_bwd_input_ln_partial(a, t):
    return _ln_fused_reads(a) + [("part", "w", a["part_bytes"])]


def _attention_fwd(a, t):
    B, N, H, hd = a["B"], a["N"], a["H"], a["hd"]
    return [("qkv", "r", B * N * 3 * H * hd * F), ("out", "w", B * N * H * hd * F), ("lse", "w", B * H * N * F)]


def _attention_bwd(a, t):
    B, N, H, hd = a["B"], a["N"], a["H"], a["hd"]
    tok = B * N * H * hd * F
    return [("qkv", "r", 3 * tok), ("out", "r", tok), ("dout", "r", tok), ("lse", "r", B * H * N * F), ("dqkv", "w", 3 * tok),
            ("delta_ws", "rw", B * H * N * F)]


def _attention_q1_fwd(a, t):
    B, N, E = a["B"], a["N"], a["H"] * a["hd"]
    return [("q", "r", B * E * F), ("kv", "r", B * N * 2 * E * F), ("o", "w", B * E * F), ("lse", "w", B * a["H"] * F)]


def _attention_q1_bwd(a, t):
    B, N, E = a["B"], a["N"], a["H"] * a["hd"]
    return [("dout", "r", B * E * F), ("o", "r", B * E * F), ("lse", "r", B * a["H"] * F), ("q", "r", B * E * F),
            ("kv", "r", B * N * 2 * E * F), ("dq", "w", B * E * F), ("dkv", "w", B * N * 2 * E * F)]


def _rows_add(a, t):
    return [("src", "r", _hull(a["rows"], a["lds"], a["cols"])), ("dst", "rw", _hull(a["rows"], a["ldd"], a["cols"]))]


def _bmu_outputs(a):
    B, K = a["B"], a["K"]
    return [("dist", "w", B * K * F), ("bmu", "w", B * 8), ("inv_nx", "w", B * F), ("inv_nw", "w", K * F), ("reranked", "rw", 4)]


def _bmu_x3_dots(a, t):
    return [("X", "r", _hull(a["B"], a["ldx"], a["L"])), ("W", "r", a["K"] * a["L"] * F), ("ws", "w", a["ws_bytes"])]


def _bmu_x3_finalize(a, t):
    return [("X", "r", _hull(a["B"], a["ldx"], a["L"])), ("W", "r", a["K"] * a["L"] * F), ("ws", "r", a["ws_bytes"])] + _bmu_outputs(a)


def _planes_floor(R, L):
    """The fragment image of a plane buffer: per 16-deep k step and 32-row block two planes of 1 KB (the norm partials
    follow it).  The extent of a plane operand that no call of the trace has written yet."""
    return ((R + 31) // 32) * ((L + 15) // 16) * 2048


def _bmu_planes_from(a, t):
    return [("src", "r", _hull(a["R"], a["ld"], a["L"])), ("planes", "w", a["planes_bytes"])]


def _adamw(a, t):
    n = a["n"]
    return [("p", "rw", n * F), ("g", "r", n * F), ("m", "rw", n * F), ("v", "rw", n * F), ("wd_per_chunk", "r", (n + 255) // 256 * F)]


def _adamw_planes(a, t):
    return _adamw(a, t) + [("planes", "w", a["planes_bytes"])]


def _bmu_planes_dots(a, t):
    return [("xplanes", "r", ("planes", _planes_floor(a["B"], a["L"]))), ("wplanes", "r", ("planes", _planes_floor(a["K"], a["L"]))),
            ("ws", "w", a["ws_bytes"])]


def _bmu_planes_finalize(a, t):
    return ([("X", "r", _hull(a["B"], a["ldx"], a["L"])), ("W", "r", a["K"] * a["L"] * F),
             ("xplanes", "r", ("planes", _planes_floor(a["B"], a["L"]))), ("wplanes", "r", ("planes", _planes_floor(a["K"], a["L"]))),
             ("ws", "r", a["ws_bytes"])] + _bmu_outputs(a))


def _som_neigh_loss(a, t):
    B, K = a["B"], a["K"]
    return [("dist", "r", B * K * F), ("bmu", "r", B * 8), ("grid", "r", K * 2 * F), ("inv_nx", "r", B * F), ("inv_nw", "r", K * F),
            ("h", "w", B * K * F), ("loss_sum", "w", F), ("coef", "w", B * K * F), ("row_dot", "w", B * F), ("col_dot", "w", K * F),
            ("ws", "rw", a["ws_bytes"])]


def _som_bwd(a, t):
    B, K, L = a["B"], a["K"], a["L"]
    return [("X", "r", _hull(B, a["ldx"], L)), ("W", "r", K * L * F), ("coef", "r", B * K * F), ("row_dot", "r", B * F),
            ("col_dot", "r", K * F), ("gW", "w", K * L * F), ("gX", "rw" if a["accumulate_gx"] else "w", _hull(B, a["ldgx"], L))]


def _l1_unpatchify(a, t):
    (n, pd), B = _patch(a), a["B"]
    img = B * a["C"] * a["S"] * a["S"] * F
    return [("pred", "r", B * (n + 1) * pd * F), ("img", "r", img), ("recon", "w", img), ("loss_sum", "w", F),
            ("dpred", "w", B * (n + 1) * pd * F), ("ws", "rw", a["ws_bytes"])]


def _cross_entropy_ls(a, t):
    B, Cn = a["B"], a["C"]
    return [("logits", "r", B * Cn * F), ("y", "r", B * 8), ("loss_sum", "w", F), ("dlogits", "w", B * Cn * F), ("ws", "rw", a["ws_bytes"])]


ACCESS = {
    "vsom_linear_fwd": _linear_fwd,
    "vsom_linear_gelu_fwd": _linear_act_fwd,
    "vsom_linear_relu_fwd": _linear_act_fwd,
    "vsom_linear_residual_fwd": _linear_residual_fwd,
    "vsom_linear_bwd_input": _linear_bwd_input("W"),
    "vsom_linear_bwd_input_t": _linear_bwd_input("Wt"),
    "vsom_transpose_many": _transpose_many,
    "vsom_linear_bwd_weight": _linear_bwd_weight,
    "vsom_patch_embed_fwd": _patch_embed_fwd,
    "vsom_patch_embed_bwd": _patch_embed_bwd,
    "vsom_layernorm_fwd": _layernorm_fwd,
    "vsom_layernorm_bwd": _layernorm_bwd,
    "vsom_layernorm_bwd_partial": _layernorm_bwd_partial,
    "vsom_layernorm_bwd_finish_many": _layernorm_bwd_finish_many,
    "vsom_linear_bwd_input_ln": _linear_bwd_input_ln,
    "vsom_linear_bwd_input_ln_partial": _linear_bwd_input_ln_partial,
    "vsom_attention_fwd": _attention_fwd,
    "vsom_attention_bwd": _attention_bwd,
    "vsom_attention_q1_fwd": _attention_q1_fwd,
    "vsom_attention_q1_bwd": _attention_q1_bwd,
    "vsom_rows_add": _rows_add,
    "vsom_bmu_cosine_x3_dots": _bmu_x3_dots,
    "vsom_bmu_cosine_x3_finalize": _bmu_x3_finalize,
    "vsom_bmu_planes_from": _bmu_planes_from,
    "vsom_adamw_step": _adamw,
    "vsom_adamw_step_planes": _adamw_planes,
    "vsom_bmu_cosine_x3_planes_dots": _bmu_planes_dots,
    "vsom_bmu_cosine_x3_planes_finalize": _bmu_planes_finalize,
    "vsom_som_neigh_loss": _som_neigh_loss,
    "vsom_som_bwd": _som_bwd,
    "vsom_l1_unpatchify": _l1_unpatchify,
    "vsom_cross_entropy_ls": _cross_entropy_ls,
    "vsom_fill": lambda a, t: [("p", "w", a["n"] * F)],
    "vsom_loss_parts": lambda a, t: [("parts", "w", 3 * F), ("main_sum", "r", F), ("som_sum", "r", F), ("counter", "rw", 8)],
    "vsom_scale_by": lambda a, t: [("p", "rw", a["n"] * F), ("scale_dev", "r", F)],
    "vsom_comm_allreduce_sum": lambda a, t: [("buf", "rw", a["n"] * F)],
    RECORD: lambda a, t: [],
    WAIT: lambda a, t: [],
}


class Incomplete(Exception):
    """A checked trace holds a launching entry with no ACCESS row, or names a device table it does not carry."""


def accesses(trace):
    """[(call index, argument name, mode, buffer, lo, hi)] of every call of the trace, by ACCESS; NULL operands and empty
    ranges are left out.  Raises Incomplete for a call with a stream that has no row."""
    tables = trace.get("tables", {})
    planes = {}                                     # pointer of a plane buffer -> the bytes its last writer gave it
    out = []
    for i, c in enumerate(trace["calls"]):
        if c["entry"] == BARRIER or c.get("stream") is None:
            continue
        row = ACCESS.get(c["entry"])
        if row is None:
            raise Incomplete("no access row for %s (step %s, position %s, stream %s)" % (c["entry"], c.get("step"), c.get("pos"), c["stream"]))
        a = c["args"]

        def table(p, nwords, _c=c):
            words = tables.get(ptr_key(p))
            if words is None or len(words) < nwords:
                raise Incomplete("%s at step %s, position %s: the trace does not carry %d words of the table at %s"
                                 % (_c["entry"], _c.get("step"), _c.get("pos"), nwords, ptr_key(p)))
            return words

        for item in row(a, table):
            name, mode, nbytes = item[0], item[1], item[2]
            base = ptr(item[4] if len(item) > 4 else a[name.split(".")[0]])
            if base is None:
                continue
            base = (base[0], base[1] + (item[3] if len(item) > 3 else 0))
            if isinstance(nbytes, tuple):                                   # a plane operand: as large as it was written
                nbytes = planes.get(base, nbytes[1])
            elif name == "planes":
                planes[base] = nbytes
            if nbytes > 0:
                out.append((i, name, mode, base[0], base[1], base[1] + nbytes))
    return out


# ------------------------------------------------------------------------------------ ordering
def _clocks(trace, skip=()):
    """Per call: (its stream, its own count on that stream, its vector clock); plus every wait's resolution.
    `skip`: indices of calls to leave out (the mutation check removes waits)."""
    clock, events, per_call, waits, floor = {}, {}, [], [], {}
    for i, c in enumerate(trace["calls"]):
        e, s = c["entry"], c.get("stream")
        if i in skip or (s is None and e != BARRIER):
            per_call.append(None)
            continue
        if e == BARRIER:
            for vc in clock.values():                # everything issued so far is complete before anything issued later
                for k, v in vc.items():
                    floor[k] = max(floor.get(k, 0), v)
            for k in clock:
                clock[k] = dict(floor)
            per_call.append(None)
            continue
        vc = clock.setdefault(s, dict(floor))
        if e == WAIT:
            rec = events.get(c["args"]["ev"])
            waits.append((i, rec[0] if rec else None))
            if rec:
                for k, v in rec[1].items():
                    if v > vc.get(k, 0):
                        vc[k] = v
        vc[s] = vc.get(s, 0) + 1
        if e == RECORD:
            events[c["args"]["ev"]] = (i, dict(vc))
        per_call.append((s, vc[s], dict(vc)))
    return per_call, waits


def _where(c):
    return "step %s #%s %s on %s" % (c.get("step"), c.get("pos"), c["entry"], c.get("stream"))


def conflict_pairs(trace):
    """[(earlier call, later call, earlier access, later access)]: pairs on different streams whose ranges overlap with at
    least one of them writing -- what has to be ordered, whatever the events do.  One entry per pair of accesses."""
    acc = sorted(accesses(trace), key=lambda x: (x[3], x[4]))
    calls = trace["calls"]
    out, active = [], []
    for x in acc:
        active = [y for y in active if y[3] == x[3] and y[5] > x[4]]
        for y in active:
            if y[0] == x[0] or calls[y[0]]["stream"] == calls[x[0]]["stream"] or (x[2] == "r" and y[2] == "r"):
                continue
            first, second = (y, x) if y[0] < x[0] else (x, y)
            out.append((first[0], second[0], first, second))
        active.append(x)
    out.sort(key=lambda p: (p[1], p[0]))
    return out


def _race(calls, first, second):
    # by what the later call does to what the earlier one did: a read-write after a write is reported as RAW
    kind = "WAR" if "w" not in first[2] else "RAW" if "r" in second[2] else "WAW"
    lo, hi = max(first[4], second[4]), min(first[5], second[5])
    a, b = calls[first[0]], calls[second[0]]
    return {"type": "race", "kind": kind, "first": first[0], "second": second[0], "first_arg": first[1], "second_arg": second[1],
            "buffer": first[3], "range": (lo, hi),
            "text": "%s race: %s (%s, %s) is not ordered before %s (%s, %s); bytes [%d, %d) of buffer %s"
                    % (kind, _where(a), first[1], first[2], _where(b), second[1], second[2], lo, hi, first[3])}


def races(trace, pairs=None, skip=()):
    pairs = conflict_pairs(trace) if pairs is None else pairs
    per_call, _ = _clocks(trace, skip)
    out = []
    for i, j, first, second in pairs:
        s, n, _ = per_call[i]
        if per_call[j][2].get(s, 0) < n:
            out.append(_race(trace["calls"], first, second))
    return out


def check(trace):
    """Every finding of the trace, in host order of the (later) call it is about."""
    calls = trace["calls"]
    out = races(trace)
    for w, r in _clocks(trace)[1]:
        if r is None:
            out.append({"type": "unrecorded-wait", "second": w,
                        "text": "%s waits for event %s, which was never recorded" % (_where(calls[w]), calls[w]["args"]["ev"])})
        elif calls[r]["stream"] == calls[w]["stream"]:
            out.append({"type": "self-wait", "first": r, "second": w,
                        "text": "%s resolves to %s, a record made on the waiting stream itself" % (_where(calls[w]), _where(calls[r]))})
    out.sort(key=lambda f: f["second"])
    return out


def wait_resolution(trace):
    """For every wait, in host order: {"wait": call index, "stream", "record": call index or None, "record_stream"} -- the
    record the wait resolves to.  Event ids are only followed, never compared: the result does not depend on which ids
    a process happened to hand out."""
    calls = trace["calls"]
    return [{"wait": w, "stream": calls[w]["stream"], "record": r, "record_stream": None if r is None else calls[r]["stream"]}
            for w, r in _clocks(trace)[1]]


def resolution_by_step(trace):
    """step -> [(ordinal of the wait among the step's waits, waiting stream, steps back to the record's step, ordinal of
    the record among that step's records, recording stream)]: wait_resolution in a form that is the same for two steps
    that synchronise alike, whatever other calls (size queries, first-step set-up) stand between the event calls."""
    calls = trace["calls"]
    ordinal, count = {}, {}
    for i, c in enumerate(calls):
        if c["entry"] in (RECORD, WAIT):
            k = (c["step"], c["entry"])
            ordinal[i] = count[k] = count.get(k, -1) + 1
    out = {}
    for r in wait_resolution(trace):
        w, rec = r["wait"], r["record"]
        row = (ordinal[w], r["stream"]) + ((None, None, None) if rec is None else
                                          (calls[w]["step"] - calls[rec]["step"], ordinal[rec], r["record_stream"]))
        out.setdefault(calls[w]["step"], []).append(row)
    return out


def describe_resolution(trace, step):
    """The step's waits as text, with call positions: what a failing comparison of resolution_by_step prints."""
    calls = trace["calls"]
    out = []
    for r in wait_resolution(trace):
        w = calls[r["wait"]]
        if w["step"] == step:
            rec = None if r["record"] is None else calls[r["record"]]
            out.append("wait #%s on %s -> %s" % (w["pos"], w["stream"], "nothing" if rec is None else
                                                 "record #%s on %s of step %s" % (rec["pos"], rec["stream"], rec["step"])))
    return out


def mutation_report(trace, step):
    """Remove each cross-stream wait of `step` in turn and check again.  -> {"waits", "load_bearing", "pairs": {(recording
    stream, waiting stream): [waits, load-bearing]}, "all_removed_races"}."""
    calls = trace["calls"]
    pairs = conflict_pairs(trace)
    cross = [r for r in wait_resolution(trace) if calls[r["wait"]]["step"] == step and r["record"] is not None
             and r["record_stream"] != r["stream"]]
    rep = {"waits": len(cross), "load_bearing": 0, "pairs": {}, "conflict_pairs": len(pairs)}
    for r in cross:
        k = (r["record_stream"], r["stream"])
        n = rep["pairs"].setdefault(k, [0, 0])
        n[0] += 1
        if races(trace, pairs, skip={r["wait"]}):
            n[1] += 1
            rep["load_bearing"] += 1
    rep["all_removed_races"] = len(races(trace, pairs, skip={i for i, c in enumerate(calls) if c["entry"] == WAIT}))
    return rep


# ------------------------------------------------------------------------------------ building traces
def call(entry, stream=None, at=0, **args):
    """One call of step `at` of a hand-written trace; `pos` is filled in by make_trace."""
    return {"step": at, "entry": entry, "stream": stream, "args": args}


def make_trace(calls, tables=None):
    pos = {}
    out = []
    for c in calls:
        c = dict(c)
        c["pos"] = pos[c["step"]] = pos.get(c["step"], -1) + 1
        out.append(c)
    return {"calls": out, "tables": dict(tables or {})}


def from_launch_fixture(case, header):
    """The trace of one case of tests/golden/step_launch_trace.json ("entry|stream|by-value arguments", no pointers): its
    host steps, then its taped steps.  Good for wait_resolution; it has no operands to check."""
    calls, step = [], 0
    for steps in (case["host_steps"], case["taped_steps"]):
        for s in steps:
            for k in s:
                entry, stream, vals = case["calls"][k].split("|")
                names = [n for n, kind in header[entry] if kind == "val"]
                vals = [float(v) if "." in v or "e" in v or "n" in v else int(v) for v in vals.split(",") if v != ""]
                calls.append(call(entry, None if stream == "-" else stream, step, **dict(zip(names, vals))))
            step += 1
    return make_trace(calls)


def _encode_case(trace, header, table, index):
    acc = accesses(trace)
    spans = sorted((b, lo, hi) for _, _, _, b, lo, hi in acc)
    merged = []
    for b, lo, hi in spans:
        if merged and merged[-1][0] == b and lo < merged[-1][2]:
            merged[-1][2] = max(merged[-1][2], hi)
        else:
            merged.append([b, lo, hi])
    number = {}

    def locate(p):
        p = ptr(p)
        if p is None:
            return "0"
        k = bisect.bisect_right(merged, [p[0], p[1], float("inf")]) - 1
        if k < 0 or merged[k][0] != p[0] or not (merged[k][1] <= p[1] < merged[k][2]):
            return "0"                               # a pointer no access row uses (an operand the entry does not touch)
        return "b%d+%d" % (number.setdefault(k, len(number)), p[1] - merged[k][1])

    first_seen = {}
    for i, _, _, b, lo, _ in acc:
        first_seen.setdefault((b, lo), i)
    for (b, lo), _ in sorted(first_seen.items(), key=lambda kv: kv[1]):
        locate((b, lo))
    steps, tables = {}, {}
    for c in trace["calls"]:
        if c["stream"] is None and c["entry"] != BARRIER:
            continue                                 # size queries, mode getters, tape control: nothing is enqueued
        text = "|".join([c["entry"], c["stream"] or "-", ",".join(
            locate(c["args"][n]) if kind == "ptr" else repr(c["args"][n]) for n, kind in header.get(c["entry"], ()) if kind != "stream")])
        if text not in index:
            index[text] = len(table)
            table.append(text)
        steps.setdefault(c["step"], []).append(index[text])
        if c["entry"] == "vsom_layernorm_bwd_finish_many":
            words = trace["tables"][ptr_key(c["args"]["jobs_dev"])]
            tables[locate(c["args"]["jobs_dev"])] = [locate(w) if k % 4 < 3 else w for k, w in enumerate(words)]
        elif c["entry"] == "vsom_transpose_many":
            tables[locate(c["args"]["table"])] = list(trace["tables"][ptr_key(c["args"]["table"])])
    return {"steps": [steps[s] for s in sorted(steps)], "tables": tables}


def encode_fixture(traces, header):
    """{case: trace} -> {"calls": one table of distinct "entry|stream|arguments in C order" for all cases, "cases": {case:
    {"steps": [[indices]], "tables": {...}}}}.  Only what a stream sees is kept (calls with a stream argument, barriers).
    Every pointer becomes b<buffer>+<offset>: a case's buffers are the connected unions of the ranges its calls touch,
    numbered by first appearance, so the text does not depend on the allocator and cases that launch alike share rows."""
    table, index = [], {}
    return {"cases": {case: _encode_case(t, header, table, index) for case, t in traces.items()}, "calls": table}


def decode_fixture(data, case, header):
    calls = []
    for step, idx in enumerate(data["cases"][case]["steps"]):
        for k in idx:
            entry, stream, vals = data["calls"][k].split("|")
            kinds = [(n, kind) for n, kind in header.get(entry, []) if kind != "stream"]
            args = {}
            for (n, kind), v in zip(kinds, [v for v in vals.split(",") if v != ""]):
                args[n] = ptr_from_key(v) if kind == "ptr" else float(v) if any(ch in v for ch in ".en") else int(v)
            calls.append(call(entry, None if stream == "-" else stream, step, **args))
    tables = {k: [ptr_from_key(w) if isinstance(w, str) else w for w in words] for k, words in data["cases"][case]["tables"].items()}
    return make_trace(calls, tables)
