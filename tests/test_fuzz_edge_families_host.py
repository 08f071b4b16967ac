"""The pinned seeds of tests/test_gpu_fuzz_edge_families.py, replayed on the CPU from the reference side alone: every case
is well-posed within the redraws (PNA within its cap of zeroed entries; the worst share is printed), the float32
restatement (the yardstick of a badly conditioned case) is finite, and together the seeds reach, for every kind, every
lane-layout class of csrc/attn_common.h the kind can take, a copied node operand and a copied per-slot operand, every row
length at the kernels' boundaries in the forward and the transposed CSR (for rgcn / film also in the relation-expanded
rows), the graphs of 1, 2 and 3 nodes, a graph without edges, every option value, parameter vectors on and off the grid,
the blocked widths and the refused ones. The class table is printed with one seed per class: break a line of a kernel or
of an op and the table names the pinned seeds whose case runs it.

The fuzz's restatement calls the host files' own `aggregate` / `operator` functions (the ones their Ref*Conv classes and
run_formula call), in the dtype of its inputs, so there is no second set of formulas that could drift from them. What
the fuzz adds is the plumbing around them: the edges in forward slot order, the per-slot rows drawn in that order, the
relation of every slot. That is checked here: in float64 the restatement over the slot order equals the restatement over
the edge list as given, with the per-slot rows carried back to it, to 1e-12 of scale (PNA's extrema send a tie's gradient
to the lowest slot, which depends on the order by design, so its gradients are left out of this one comparison)."""
import functools

import torch

import test_gpu_fuzz_edge_families as EF
from test_fuzz_families_host import ROW_CLASSES, row_classes
from test_gpu_fuzz_families import as_kernel_sees, make_layout, min_vec, vec_by_width

T = EF.T
HEAD_KINDS = ("resgated", "softmax", "gine", "cgconv", "rgcn", "film", "gmm")   # kernels on attn_common.h's lane layout
LAYOUT_CLASSES = ("vec4 by C", "vec2 by C", "vec1 by C", "vec lowered by an operand, C % 4 == 0", "lanes beyond C",
                  "idle lanes in a group", "one head chunk", "several chunks, full last", "several chunks, partial last",
                  "LPH = 64", "G = 1", "node operand copied to fit a wave")
ONE_HEAD = {"idle lanes in a group", "several chunks, full last", "several chunks, partial last"}
# rgcn's mix form has B in {1, 2, 4} heads: HPC is a power of two that divides B, so no idle lanes and no partial chunk
NOT_FOR = {"resgated": ONE_HEAD, "softmax": ONE_HEAD, "gine": ONE_HEAD, "cgconv": ONE_HEAD, "film": ONE_HEAD,
           "rgcn": {"idle lanes in a group", "several chunks, partial last"}}
SLOT_COPY = "per-slot operand copied to fit a wave"
LEAVES = {"resgated": ["k", "q", "v"], "softmax": ["m", "t"], "gine": ["x", "e", "eps"], "cgconv": ["a", "b", "c", "root"],
          "rgcn": ["h", "y0", "comp"], "film": ["h", "fb", "y0"], "gmm": ["h", "e", "y0", "mu", "sigma"],
          "pna": ["a", "b", "c"], "bf16": ["x", "bias"]}
WITH_VECTORS = ("softmax", "gine", "rgcn", "gmm", "bf16")


def test_long_row_slots_is_the_package_constant():
    from rgb_experiment_amd import graph
    assert graph.LONG_ROW_SLOTS == T
    assert (graph.LOOPS_KEEP, graph.LOOPS_ADD_REMAINING) == (EF.LOOPS_KEEP, EF.LOOPS_ADD_REMAINING)


def head_operands(c):
    """[(name, rows, width, copied by .contiguous() first)] of the matrices a head kernel's pick_vec counts."""
    kind, n, E, C = c["kind"], c["n"], c["E"], c["C"]
    if kind == "film":   # several relations: h and fb pass .contiguous().view(N * R, .) first
        wide = c["R"] > 1
        ops = [("h", n, c["R"] * C, wide), ("fb", n, 2 * c["R"] * C, wide)]
    elif kind == "rgcn":
        ops = [("h", n, c["B"] * C, False)]
    elif kind == "gmm":
        ops = [("h", n, c["K"] * C, False)]          # e is read one float at a time
    elif kind == "cgconv":
        ops = [("a", n, 2 * C, False), ("b", n, 2 * C, False), ("c", E, 2 * C, False), ("root", n, C, False)]
    else:
        ops = [(m, E if m in c["slot_mats"] else n, C, False) for m in c["mats"]]
    ops.append(("y0", n, C, False))
    return [o for o in ops if o[0] in c["mats"]]


def layout_classes(c):
    """The lane-layout classes a case of a head kernel runs at (one launch: C <= 256, form mix for rgcn). The ops copy an
    operand off the grid of min_vec(C) (ops._rows_on_grid); pick_vec then takes the widest of 4, 2 that divides C and that
    every operand's pointer and leading dimension allow."""
    kind, C = c["kind"], c.get("C")
    if kind not in HEAD_KINDS or c["refused"] or C > 256 or (kind == "rgcn" and c["form"] == "select"):
        return set()
    H = {"rgcn": c.get("B"), "gmm": c.get("K")}.get(kind, 1)
    got, vec, grid = set(), vec_by_width(C), min_vec(C)
    for name, rows, width, copies in head_operands(c):
        off, ld = as_kernel_sees(c["layouts"][name], rows, width, copies)
        if rows == 0:
            continue
        if off % grid or ld % grid:
            got.add(SLOT_COPY if name in c["slot_mats"] else "node operand copied to fit a wave")
            continue
        while vec > 1 and (off % vec or ld % vec):
            vec //= 2
    lph, hpc, G = make_layout(H, C, vec)
    chunks = (H + hpc - 1) // hpc
    if vec == vec_by_width(C):
        got.add(f"vec{vec} by C")
    elif C % 4 == 0:
        got.add("vec lowered by an operand, C % 4 == 0")
    if lph * vec > C:
        got.add("lanes beyond C")
    if hpc * lph < G:
        got.add("idle lanes in a group")
    if chunks == 1:
        got.add("one head chunk")
    else:
        got.add("several chunks, full last" if H - (chunks - 1) * hpc == hpc else "several chunks, partial last")
    if lph == 64:
        got.add("LPH = 64")
    if G == 1:
        got.add("G = 1")
    return got


def pna_classes(c):
    """PNA's operands go on the grid of four floats whatever the width; d above 256 is cut at tower boundaries."""
    got = set()
    if c["refused"]:
        return got
    for m in c["mats"]:
        rows = c["E"] if m in c["slot_mats"] else c["n"]
        off, ld = as_kernel_sees(c["layouts"][m], rows, c["d"], False)
        if rows and (off % 4 or ld % 4):
            got.add(("per-slot" if m in c["slot_mats"] else "node") + " operand copied onto the grid of 4")
    blocks = EF.pna_blocks(c["d"], c["F"])
    if len(blocks) > 1:
        got.add("d above 256: several launches")
        if 256 % c["F"]:
            got.add("d above 256, cut before column 256 (F does not divide 256)")
        if blocks[-1][1] - blocks[-1][0] < blocks[0][1] - blocks[0][0]:
            got.add("d above 256, a narrower last launch")
    return got


def option_values(c):
    kind = c["kind"]
    got = {("run", c["run"]), ("cotangent", c["cot"]), ("graph", c["style"])}
    got |= {("layout", c["layouts"][m][0]) for m in c["mats"]}
    got |= {("slot layout", c["layouts"][m][0]) for m in c["slot_mats"]}
    if c["run"] != "no_grad":
        got |= {("grad " + k, k in c["req"]) for k in c["mats"] + c["vecs"]}
    got.add(("refused", c["refused"]))
    if c["vecs"] or c.get("eps_form") == "fixed":
        got.add(("parameter vector off the grid", c["vec_off"] > 0))
    for k in ("t_form", "eps_form", "aggr", "with_c", "with_root", "with_a", "with_y0", "form", "R", "B", "et_style", "typed",
              "act", "K", "D", "degree_pseudo", "towers", "agg", "op", "addend", "bias", "transposed", "out_dtype"):
        if k in c:
            got.add((k, c[k]))
    if kind == "softmax" and c["t_form"] == "scalar":
        got.add(("t_value", c["t_value"]))
    if kind in EF.BLOCKED and c["C"] > 256:
        got.add(("blocked width", c["C"]))
        if kind == "film":
            got.add(("blocked branch", "one view (C % 4 == 0)" if c["C"] % 4 == 0 else "torch.cat (C % 4 != 0)"))
    if kind in EF.TYPED and c["R"] > 1:
        got.add(("a relation without edges", True))
    if kind in ("rgcn", "film") and c.get("form", "select") == "select" and c.get("typed", True) and c["aggr"] == "mean" \
            and c["run"] != "no_grad" and "h" in c["req"] and c["R"] > 1 and not c["refused"]:
        got.add(("g_h over the relation-expanded transposed CSR, mean weights", True))
    if kind == "pna":
        got |= {("aggregator", a) for a in c["aggrs"]} | {("scaler", s) for s in c["scalers"]}
    if kind == "bf16":
        got.add(("width", c["d"]))
    return got


def required_options(kind):
    need = {("run", "no_grad"), ("run", "eval"), ("cotangent", "dense"), ("cotangent", "stride2"), ("cotangent", "block"),
            ("graph", "prescribed"), ("graph", "random"), ("layout", "fresh"), ("layout", "block"), ("layout", "offset")}
    need |= {("grad " + k, v) for k in LEAVES[kind] for v in (True, False)}
    if kind != "bf16":
        need |= {("refused", True), ("refused", False)}
    if kind in WITH_VECTORS:
        need |= {("parameter vector off the grid", True), ("parameter vector off the grid", False)}
    if kind in ("gine", "cgconv", "gmm", "pna"):
        need |= {("slot layout", v) for v in ("fresh", "block", "offset")}
    both = lambda k: {(k, True), (k, False)}
    if kind == "softmax":
        need |= {("t_form", "scalar"), ("t_form", "channel")} | {("t_value", v) for v in ("zero", "negative", "range")}
    if kind == "gine":
        need |= {("eps_form", v) for v in (None, "fixed", "learned")} | {("blocked width", w) for w in (260, 300, 512)}
    if kind == "cgconv":
        need |= {("aggr", "add"), ("aggr", "mean")} | both("with_c") | both("with_root")
    if kind == "rgcn":
        need |= {("form", "select"), ("form", "mix")} | {("R", r) for r in (1, 2, 3, 5, 8)} | {("B", b) for b in (1, 2, 4)}
    if kind == "film":
        need |= both("typed") | {("R", r) for r in (1, 2, 4)} | {("act", "relu"), ("act", "identity")}
        need |= {("blocked width", 258), ("blocked width", 300), ("blocked branch", "one view (C % 4 == 0)"),
                 ("blocked branch", "torch.cat (C % 4 != 0)")}
    if kind in ("rgcn", "film"):
        need |= {("aggr", "mean"), ("aggr", "add")} | both("with_y0")
        need |= {("et_style", s) for s in ("by_target", "by_source", "uniform")}
        need |= {("a relation without edges", True), ("g_h over the relation-expanded transposed CSR, mean weights", True)}
    if kind == "gmm":
        need |= {("K", k) for k in EF.GMM_K} | {("D", d) for d in EF.GMM_D} | both("degree_pseudo") | both("with_y0")
        need |= {("aggr", "mean"), ("aggr", "add")}
    if kind == "pna":
        import test_pna_host as PH
        need |= {("aggregator", a) for a in PH.AGGREGATORS} | {("scaler", s) for s in PH.SCALERS}
        need |= both("with_a") | both("with_c")
        need |= {("towers", t) for t in (1, 2, 3, 4)}
    if kind == "bf16":
        need |= {("agg", a) for a in ("gcn", "mean", "sum")} | {("op", o) for o in ("rows", "any", "raw")} | both("addend")
        need |= both("bias") | both("transposed") | {("out_dtype", "fp32"), ("out_dtype", "bf16")}
        need |= {("width", w) for w in EF.BF16_WIDTHS + EF.ANY_WIDTHS}
    return need


def required_classes(kind):
    need = []
    if kind in HEAD_KINDS:
        need += [cls for cls in LAYOUT_CLASSES if cls not in NOT_FOR.get(kind, ())]
    if kind in ("gine", "cgconv"):
        need.append(SLOT_COPY)
    if kind == "pna":
        need += ["node operand copied onto the grid of 4", "per-slot operand copied onto the grid of 4",
                 "d above 256: several launches", "d above 256, cut before column 256 (F does not divide 256)",
                 "d above 256, a narrower last launch"]
    for side in ("forward", "transposed"):
        need += [f"{side} row of {cls}" for cls in ROW_CLASSES]
    if kind in EF.TYPED:
        for side in ("forward", "transposed"):
            need += [f"relation-expanded {side} row of {cls}" for cls in ROW_CLASSES]
    need += [f"n = {n}" for n in (1, 2, 3)] + ["a graph without edges"]
    if kind in ("gine", "cgconv", "gmm", "pna"):
        need.append("a graph without edges, the per-slot operand given")
    if kind == "softmax":
        need.append("cotangent zeroed on a row of 256 or more copies of one edge")
    return need + [f"{opt} = {val}" for opt, val in sorted(required_options(kind), key=str)]


@functools.lru_cache(maxsize=None)
def replay():
    """kind -> {class -> [seeds]} over the pinned seeds, the problems met on the way, and PNA's worst zeroed share."""
    table = {k: {} for k in EF.KINDS}
    problems, worst = [], (0.0, None)
    for seed in EF.pinned_seeds():
        c = EF.draw_case(seed)
        kind, n = c["kind"], c["n"]

        def hit(name):
            seeds = table[kind].setdefault(name, [])
            if seed not in seeds:
                seeds.append(seed)
        try:
            data, want64, redraws = EF.posed_data(c)
        except AssertionError as exc:
            problems.append(str(exc))
            continue
        if data.get("share", 0.0) > worst[0]:
            worst = (data["share"], seed)
        if want64 is not None:
            want32 = EF.reference(c, data, torch.float32)
            given = EF.reference(dict(c, edge_order="given"), data)
            for name, ref in want64.items():
                if ref is None:
                    if want32[name] is not None or given[name] is not None:
                        problems.append(f"{c['desc']}: {name} is None in one restatement only")
                    continue
                if not ref.numel():
                    continue
                scale = max(1.0, ref.abs().max().item())
                own = (want32[name].double() - ref).abs().max().item()
                if not (own == own and own != float("inf")):
                    problems.append(f"{c['desc']}: the float32 restatement of {name} is not finite")
                tol = EF.FWD_TOL if name == "out" else EF.GRAD_TOL
                if EF.FF.OWN_FACTOR * own > tol * scale:
                    hit("ill-conditioned (the float32 restatement sets the bar)")
                # (the gradient of a per-slot operand is taken at the slot-ordered leaf in both: nothing to permute)
                if not (kind == "pna" and name != "out") and (given[name] - ref).abs().max().item() > 1e-12 * scale:
                    problems.append(f"{c['desc']}: {name} over the slot order differs from {name} over the edge list as given")
        if redraws:
            hit("data redrawn")
        if kind == "softmax":
            dup = EF.FF.duplicate_rows(dict(c, kind="transformer"))
            if bool(dup.any()):
                hit("cotangent zeroed on a row of 256 or more copies of one edge")
                if float(data["cot"][dup].abs().max()) != 0.0:
                    problems.append(f"{c['desc']}: the cotangent of the duplicate rows")
        if kind == "pna" and data.get("share", 0.0) > 0.0:
            hit("cotangent zeroed at a near-tie or in the variance band")
        for cls in layout_classes(c) | (pna_classes(c) if kind == "pna" else set()):
            hit(cls)
        fwd, bwd = EF.row_lengths(c["ei"], n, c["mode"])
        for cls in row_classes(fwd):
            hit("forward row of " + cls)
        for cls in row_classes(bwd):
            hit("transposed row of " + cls)
        if kind in EF.TYPED and c.get("typed", True) and not c["refused"]:
            R, et = c["R"], c["et"]
            for cls in row_classes(torch.bincount(c["ei"][1] * R + et, minlength=n * R)):
                hit("relation-expanded forward row of " + cls)
            for cls in row_classes(torch.bincount(c["ei"][0] * R + et, minlength=n * R)):
                hit("relation-expanded transposed row of " + cls)
        if n <= 3:
            hit(f"n = {n}")
        if c["E"] == 0:
            hit("a graph without edges")
            if c["slot_mats"] and not c["refused"]:
                hit("a graph without edges, the per-slot operand given")
        for opt, val in option_values(c):
            hit(f"{opt} = {val}")
    return table, problems, worst


def test_every_pinned_case_is_well_posed_and_its_float32_yardstick_finite():
    _, problems, worst = replay()
    print(f"\npna: the worst share of zeroed entries in the max / min / var / std blocks is {worst[0]:.4f} (seed {worst[1]}), "
          f"cap {EF.PNA_CAP}")
    assert worst[0] <= EF.PNA_CAP
    assert not problems, "\n".join(problems)


def test_pinned_seeds_reach_every_class_for_every_kind():
    table, _, _ = replay()
    missing = []
    for kind in EF.KINDS:
        need = required_classes(kind)
        print(f"\n{kind}: {len([s for s in EF.pinned_seeds() if EF.KINDS[s % len(EF.KINDS)] == kind])} pinned cases")
        for cls in need + sorted(set(table[kind]) - set(need)):
            seeds = table[kind].get(cls, [])
            print(f"  {cls:66s} {len(seeds):3d}  {seeds[:6]}")
            if not seeds:
                missing.append((kind, cls))
    assert not missing, missing


def test_the_draw_needs_no_device_and_repeats():
    a, b = EF.draw_case(1234), EF.draw_case(1234)
    assert a["desc"] == b["desc"] and torch.equal(a["ei"], b["ei"])
    assert [EF.draw_case(s)["kind"] for s in range(len(EF.KINDS))] == EF.KINDS
    assert EF.draw_case(5, "pna")["kind"] == "pna"
