"""The two-stream pipelined step of bench.py (`instrumented_step` under --overlap), restated so that tests can run it and reason about it:

  * pipelined_steps: the same engine calls in the same order behind the same events, fed a DIFFERENT frame batch per step and returning every
    step's outputs (the benchmark feeds every step the same frames and keeps the last step's);
  * ACCESS: for every engine call of the step, the handle-owned workspace regions it reads and writes, read off capi.cpp by hand;
  * choreography / unroll / conflicts: the ordered stream operations of a step function taken from its source with `ast`, unrolled over several
    steps into (step, call, stream) operations, and a happens-before check of ACCESS over them (stream order + event record -> wait).

tests/test_two_stream_step_cpu.py holds the table and the choreography together without a GPU; tests/test_gpu_two_stream_step.py runs
pipelined_steps on one.  include/semdepth.h ("Streams") states the contract both check."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "semantic_depth_amd", "csrc", "capi.cpp")
ARENA = os.path.join(ROOT, "semantic_depth_amd", "csrc", "handle_arena.hpp")
BENCH = os.path.join(ROOT, "bench.py")
HEADER = os.path.join(ROOT, "include", "semdepth.h")


# ------------------------------------------------------------------------------------------------------------------ the step, restated
def pipelined_steps(eng, batches, cams, prm, approach, colours, side_priority):
    """bench.py's instrumented_step with a side stream, once per batch of ``batches`` (u8 [B,H,W,3] device tensors, B may change from step to
    step; ``cams``: one Camera per frame of the largest batch).  The two networks of step i+1 go onto the current stream, the tail of step i
    (fuse_from_raw -> road_width -> fence_to_fence) onto a side stream of priority ``side_priority``; ev[3] and ev[4] order the raw disparity
    pair in the activation arena.  No host synchronisation: the caller synchronises once before it reads the returned per-step outputs."""
    import torch
    from semantic_depth_amd.engine import FenceParams
    ev = [torch.cuda.Event() for _ in range(7)]
    side = torch.cuda.Stream(priority=side_priority)
    fused_once = False
    outs = []
    for fr in batches:
        cams_b = cams[:fr.shape[0]]
        ev[0].record()
        ev[1].record()
        seg = eng.fcn8s_forward(fr)
        ev[2].record()
        if fused_once:
            torch.cuda.current_stream().wait_event(ev[4])      # the previous step's fusion stage has consumed the raw pair in the arena
        eng.monodepth_forward(fr, post_process=False)          # the raw pair stays in the arena for the one-pass fusion stage
        ev[3].record()
        side.wait_event(ev[3])
        for t_ in (seg["road"], seg["fence"], fr):
            t_.record_stream(side)
        ctx = torch.cuda.stream(side)
        with ctx:
            fz = eng.fuse_from_raw(seg["road"], seg["fence"], fr, cams_b, want_rgb=colours)
            ev[4].record()
            fused_once = True
            rec = eng.road_width(fz["road_xyz"], fz["n_road"], prm, road_rgb=fz["road_rgb"] if colours else None)
            ev[5].record()
            f2f = None
            if approach == "both":
                f2f = eng.fence_to_fence(fz["fence_xyz"], fz["n_fence"], rec, FenceParams(depth=prm.depth),
                                         fence_rgb=fz["fence_rgb"] if colours else None)
            ev[6].record()
        outs.append(dict(seg=seg, disp_pp=fz["disp_pp"], fuse=fz, records=rec, f2f=f2f))
    return outs


# ------------------------------------------------------------------------------------------------------------------ the access table
# Every region struct Arena (csrc/handle_arena.hpp) takes, at its granularity; o_misc by its parts (regions of their own there), the raw disparity pair as
# a region of its own inside o_mono.  "who": the call families of semdepth.h's Streams paragraph.
REGIONS = {
    "o_fcn": "FCN-8s activations",
    "o_mono": "monodepth activations (without the raw pair)",
    "o_mono.raw_pair": "the monodepth plan's output tensor: the raw disparity pair the one-pass fusion reads from the arena",
    "o_fuse": "block counts / offsets of the count-scan-write fusion forms",
    "o_fuse1": "look-back words and tickets of the one-pass fusion (epoch on the host: sd_handle::fuse_epoch)",
    "o_cams": "device copy of the cameras of the last fusion",
    "o_bufA": "point ping-pong A of the road and fence chains",
    "o_bufB": "point ping-pong B of the road and fence chains",
    "o_rgbA": "colour ping-pong A",
    "o_rgbB": "colour ping-pong B",
    "o_cnt": "per-stage point counts: slots 1-6 road chain, 8-14 fence chain",
    "o_plane": "road plane coefficients",
    "o_o3d": "Open3D filter scratch; left fence cloud of the fence chain",
    "o_misc.scalar": "+0: the point count of the single-cloud sd_pcl_* / sd_o3d_* calls",
    "o_misc.zero_page": "+256 .. +4096: zeros the convolutions read for padding taps; written by sd_bind_memory alone",
    "o_misc.f2f_counts": "+4096: the packed [7][B] counts of sd_fence_to_fence",
    "o_misc.f2f_planes": "road | left | right plane coefficients of sd_fence_to_fence",
    "o_misc.clamp_counters": "fp16 clamp counters: global, per image, per frame, unowned",
    "o_cmp": "ordered-compaction scratch of the road chain",
    "o_rsz": "tap tables of sd_resize_cubic_u8",
    "o_rsz_cmp": "tap tables of sd_compose_result_frames",
    "o_splitk": "partial sums of the split layers (sd_set_small_batch handles)",
}

_CHAIN = {"o_bufA", "o_bufB", "o_rgbA", "o_rgbB", "o_cnt", "o_o3d"}
# engine call -> regions read / written, and the capi.cpp function(s) they were read from
ACCESS = {
    "fcn8s_forward": dict(
        cite="sd_fcn8s_forward -> run_plan (c.zero16, c.sat, c.partial, launch_sat_fold); Engine._post_range_check -> sd_saturation_count_async",
        reads={"o_fcn", "o_misc.zero_page", "o_misc.clamp_counters", "o_splitk"},
        writes={"o_fcn", "o_misc.clamp_counters", "o_splitk"}),
    "monodepth_forward": dict(
        cite="sd_monodepth_forward -> run_plan (c.zero16, c.sat, c.partial, launch_sat_fold; p.t_output is the raw pair); "
             "Engine._post_range_check -> sd_saturation_count_async",
        reads={"o_mono", "o_misc.zero_page", "o_misc.clamp_counters", "o_splitk"},
        writes={"o_mono", "o_mono.raw_pair", "o_misc.clamp_counters", "o_splitk"}),
    "fuse_from_raw": dict(
        cite="sd_postprocess_fuse_backproject (disp_raw == NULL: the arena's pair) -> fuse_impl (dcams, blk_counts, lb_state, lb_ticket, hipMemsetAsync)",
        reads={"o_mono.raw_pair", "o_cams", "o_fuse", "o_fuse1"},
        writes={"o_cams", "o_fuse", "o_fuse1"}),
    "road_width": dict(
        cite="sd_road_width (A, B2, cA, cB, cnt_slot 1-6, plane, o3d, cmp)",
        reads=_CHAIN | {"o_plane", "o_cmp"},
        writes=_CHAIN | {"o_plane", "o_cmp"}),
    "fence_to_fence": dict(
        cite="sd_fence_to_fence (A, Rb, Lb / cL in o_o3d, cA, cR, cnt_slot 8-14, packed, planes)",
        reads=_CHAIN | {"o_misc.f2f_counts", "o_misc.f2f_planes"},
        writes=_CHAIN | {"o_misc.f2f_counts", "o_misc.f2f_planes"}),
}


def carved_regions(path=ARENA):
    """every region struct Arena takes (its `<field> = take(` declarations), under the name semdepth.h documents it by: o_<field>, and o_misc for
    the five fields the header lists as its parts"""
    src = open(path).read()
    arena = src[src.index("struct Arena :"):]
    misc = {"scalar", "zero", "f2f_counts", "f2f_planes", "sat"}
    names = ["o_misc" if f in misc else "o_" + f for f in re.findall(r"\b(\w+) = take\(", arena[:arena.index("};")])]
    return list(dict.fromkeys(names))


# ------------------------------------------------------------------------------------------------------------------ choreography from source
_STREAMS = {"torch.cuda.current_stream()": "main", "side": "side"}


def _function(path_or_source, name):
    src = open(path_or_source).read() if os.path.exists(path_or_source) else path_or_source
    found = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1, (name, len(found))
    return found[0]


def _ev_index(node):
    if isinstance(node, ast.Subscript) and isinstance(node.value, ast.Name) and node.value.id == "ev" and isinstance(node.slice, ast.Constant):
        return node.slice.value
    return None


def choreography(path_or_source, name):
    """the ordered stream operations of function ``name``, in source order:
    ("eng", method) | ("wait", "main" | "side", k) | ("record", k) | ("record_stream", stream) | ("stream", stream) | ("with",) | ("end_with",)"""
    out = []

    class V(ast.NodeVisitor):
        def visit_With(self, node):
            for it in node.items:
                self.visit(it)
            out.append(("with",))                       # enters the context of the last ("stream", s)
            for s in node.body:
                self.visit(s)
            out.append(("end_with",))

        def visit_Call(self, node):
            f = node.func
            if isinstance(f, ast.Attribute):
                recv = ast.unparse(f.value)
                if recv == "eng":
                    out.append(("eng", f.attr))
                elif f.attr == "wait_event":
                    out.append(("wait", _STREAMS[recv], _ev_index(node.args[0])))
                elif f.attr == "record_stream":
                    out.append(("record_stream", ast.unparse(node.args[0])))
                elif f.attr == "record" and _ev_index(f.value) is not None:
                    out.append(("record", _ev_index(f.value)))
                elif ast.unparse(f) == "torch.cuda.stream":
                    out.append(("stream", ast.unparse(node.args[0])))
            self.generic_visit(node)

    V().visit(_function(path_or_source, name))
    return out


def bench_choreography():
    """instrumented_step of bench.py, without the config-5 resize (gather_records is no stream operation of the engine)"""
    return [op for op in choreography(BENCH, "instrumented_step") if op != ("eng", "resize_cubic")]


# ------------------------------------------------------------------------------------------------------------------ happens-before
def unroll(chor, steps, approach="both"):
    """``steps`` repetitions of a step's choreography as operations dict(step, kind, name, stream, preds): an engine call, an event record or
    an event wait, each on the stream it is enqueued on; preds = the operation before it on its stream, and for a wait the last record of its
    event in host order (a wait on an event never recorded is a no-op, as in HIP)."""
    ops, last_on, last_record = [], {}, {}

    def add(step, kind, name, stream, extra=()):
        preds = [p for p in (last_on.get(stream), *extra) if p is not None]
        ops.append(dict(step=step, kind=kind, name=name, stream=stream, preds=preds))
        last_on[stream] = len(ops) - 1
        return len(ops) - 1

    for step in range(steps):
        cur, stack, pending = "main", [], None
        for op in chor:
            if op[0] == "stream":
                pending = op[1]
            elif op[0] == "with":
                stack.append(cur)
                cur, pending = (pending or cur), None
            elif op[0] == "end_with":
                cur = stack.pop()
            elif op[0] == "eng":
                if op[1] == "fence_to_fence" and approach != "both":
                    continue
                add(step, "call", op[1], cur)
            elif op[0] == "record":
                last_record[op[1]] = add(step, "record", op[1], cur)
            elif op[0] == "wait":
                add(step, "wait", op[2], op[1], (last_record.get(op[2]),))
        assert not stack
    return ops


def conflicts(ops, access=ACCESS):
    """[(region, earlier call, later call)] as (step, name, stream) triples: two accesses to one region, at least one a write, neither ordered
    before the other.  Host order is a topological order of the edges, so ancestors are one forward pass of bit sets."""
    anc = []
    for i, o in enumerate(ops):
        a = 0
        for p in o["preds"]:
            a |= anc[p] | (1 << p)
        anc.append(a)
    calls = [i for i, o in enumerate(ops) if o["kind"] == "call"]
    bad = []
    for x, i in enumerate(calls):
        ai = access[ops[i]["name"]]
        for j in calls[x + 1:]:
            if (anc[j] >> i) & 1:
                continue
            aj = access[ops[j]["name"]]
            for region in sorted((ai["writes"] & (aj["reads"] | aj["writes"])) | (aj["writes"] & ai["reads"])):
                bad.append((region, *[(ops[k]["step"], ops[k]["name"], ops[k]["stream"]) for k in (i, j)]))
    return bad
