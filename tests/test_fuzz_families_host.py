"""The pinned seeds of tests/test_gpu_fuzz_families.py, replayed on the CPU from the reference side alone: every case is
well-posed within the redraws, the float32 restatement (the yardstick of a badly conditioned case) is finite and the
generic-dtype restatement equals the suite's in float64, and together the seeds reach every lane-layout class of
csrc/attn_common.h, every row length at the kernels' boundaries in the forward and the transposed CSR, the graphs of
1, 2 and 3 nodes and every option value, for every kind. The class table is printed, with one seed per class: break a
line of a kernel and the table names the pinned seeds whose case runs it."""
import functools

import torch

import test_gpu_fuzz_families as FF

T = FF.T
LAYOUT_CLASSES = ("vec4 by C", "vec2 by C", "vec1 by C", "vec lowered by an operand, C % 4 == 0", "lanes beyond C",
                  "idle lanes in a group", "one head chunk", "several chunks, full last", "several chunks, partial last",
                  "LPH = 64", "G = 1", "operand copied to fit a wave")
# FAConv has one head (no chunks, no idle lanes: G = LPH) and takes its vector width from C alone
NOT_FOR = {"faconv": {"vec lowered by an operand, C % 4 == 0", "idle lanes in a group", "several chunks, full last",
                      "several chunks, partial last"}}
ROW_CLASSES = ("0", "1", "64", "65", "T", "T + 1", "one-slot last chunk", "three or more chunks")


def test_long_row_slots_is_the_package_constant():
    from rgb_experiment_amd import graph
    assert graph.LONG_ROW_SLOTS == T
    assert (graph.LOOPS_KEEP, graph.LOOPS_ADD_REMAINING, graph.LOOPS_REMOVE_ADD) == (0, 1, 2)


def layout_classes(c):
    lc = FF.layout_class(c)
    if lc is None:
        return set()
    C, vec = c["C"], lc["vec"]
    got = set()
    if not lc["lowered"]:
        got.add(f"vec{vec} by C")
    elif C % 4 == 0:
        got.add("vec lowered by an operand, C % 4 == 0")
    if lc["LPH"] * vec > C:
        got.add("lanes beyond C")
    if lc["HPC"] * lc["LPH"] < lc["G"]:
        got.add("idle lanes in a group")
    if lc["chunks"] == 1:
        got.add("one head chunk")
    else:
        got.add("several chunks, full last" if lc["last"] == lc["HPC"] else "several chunks, partial last")
    if lc["LPH"] == 64:
        got.add("LPH = 64")
    if lc["G"] == 1:
        got.add("G = 1")
    grid = FF.vec_by_width(C) if c["kind"] == "faconv" else FF.min_vec(C)
    for m in c["mats"]:
        off, ld = FF.as_kernel_sees(c["layouts"][m], c["n"], c["H"] * C, copies=c["kind"] in ("supergat", "faconv"))
        if grid > 1 and (off % grid or ld % grid):
            got.add("operand copied to fit a wave")
    return got


def row_classes(lengths):
    got = set()
    for v in set(lengths.tolist()):
        for name, hit in (("0", v == 0), ("1", v == 1), ("64", v == 64), ("65", v == 65), ("T", v == T),
                          ("T + 1", v == T + 1), ("one-slot last chunk", v > T and v % T == 1),
                          ("three or more chunks", v > 2 * T)):
            if hit:
                got.add(name)
    return got


def option_values(c):
    """(option, value) pairs a case contributes; REQUIRED lists what every kind must show."""
    kind = c["kind"]
    got = {("run", c["run"]), ("cotangent", c["cot"]), ("graph", c["style"])}
    got |= {("layout", c["layouts"][m][0]) for m in c["mats"]}
    got |= {("grad " + k, k in c["req"]) for k in c["mats"] + c["vecs"]}
    if c["run"] == "train":
        got.add(("p_drop", c["p_drop"]))
    for k in ("refused", "form", "eps", "pos_ratio", "op", "bag_of_words"):
        if k in c:
            got.add((k, c[k]))
    if kind in ("gatv2", "supergat", "gru", "weighted"):
        got.add(("bias", c["bias"]))
    if kind in ("gatv2", "transformer", "supergat"):
        got.add(("concat", c["concat"]))
    if kind == "transformer":
        got.add(("scale", ("1/sqrt(C)", "1/C", "0.37")[[1.0 / c["C"] ** 0.5, 1.0 / c["C"], 0.37].index(c["scale"])]))
    if kind == "gru":
        got.add(("padded", c["Cp"] != c["C"]))
        got.add(("fused width", c["Cp"] % 8 == 0 and c["Cp"] <= 64))
    if kind == "multi":
        got |= {("aggr", a) for a in c["aggrs"]}
        got.add(("several aggrs", len(c["aggrs"]) > 1))
    return got


def required_options(kind):
    need = {("run", "no_grad"), ("run", "eval"), ("cotangent", "dense"), ("cotangent", "stride2"), ("cotangent", "block"),
            ("graph", "prescribed"), ("graph", "random"), ("layout", "fresh"), ("layout", "block"), ("layout", "offset")}
    if kind in FF.ATTENTION:
        need |= {("run", "train")} | {("p_drop", p) for p in FF.P_DROP} | {("refused", True), ("refused", False)}
    leaves = {"gatv2": ["xl", "xr", "att", "bias"], "transformer": ["q", "k", "v"],
              "supergat": ["h", "att_l", "att_r", "bias"], "faconv": ["x", "x0", "att_l", "att_r"],
              "gru": ["x", "weight", "w_ih", "w_hh", "b_ih", "b_hh"], "extremum": [], "multi": [],
              "weighted": ["x", "ew", "W", "bias"]}[kind]
    need |= {("grad " + k, v) for k in leaves for v in (True, False)}
    if kind in ("gatv2", "supergat", "gru", "weighted"):
        need |= {("bias", True), ("bias", False)}
    if kind in ("gatv2", "transformer", "supergat"):
        need |= {("concat", True), ("concat", False)}
    if kind == "transformer":
        need |= {("scale", s) for s in ("1/sqrt(C)", "1/C", "0.37")}
    if kind == "supergat":
        need |= {("pos_ratio", 1.0), ("pos_ratio", 0.8)}
    if kind == "faconv":
        need |= {("form", f) for f in (None, "fused", "composed")} | {("eps", e) for e in (0.0, 0.1, 0.3)}
    if kind == "gru":
        need |= {("form", f) for f in (None, "fused", "composed", "general")} | {("padded", True), ("padded", False),
                                                                              ("fused width", True), ("fused width", False)}
    if kind == "extremum":
        need |= {("op", "max"), ("op", "min"), ("bag_of_words", True), ("bag_of_words", False)}
    if kind == "multi":
        need |= {("aggr", a) for a in FF.STATS} | {("several aggrs", True), ("several aggrs", False)}
    if kind == "weighted":
        need |= {("op", "gcn"), ("op", "appnp"), ("op", "sgc")}
    return need


@functools.lru_cache(maxsize=None)
def replay():
    """kind -> {class -> [seeds]} over the pinned seeds, with the per-case checks made on the way."""
    table = {k: {} for k in FF.KINDS}
    problems = []
    for seed in FF.pinned_seeds():
        c = FF.draw_case(seed)
        kind, n = c["kind"], c["n"]
        def hit(name):
            seeds = table[kind].setdefault(name, [])
            if seed not in seeds:
                seeds.append(seed)
        try:
            data, _, redraws = FF.posed_data(c)
        except AssertionError as exc:
            problems.append(str(exc))
            continue
        choices = FF.synthetic_choices(c, seed) if c["run"] == "train" else None
        want64 = FF.reference(c, data, choices)
        generic64 = FF.reference(c, data, choices, torch.float64, suite=False)
        want32 = FF.reference(c, data, choices, torch.float32)
        fwd_tol, grad_tol = FF.bars(c)
        for name, ref in want64.items():
            if name == "s":
                continue
            if ref is None:
                if generic64[name] is not None or want32[name] is not None:
                    problems.append(f"{c['desc']}: {name} is None in one restatement only")
                continue
            if not ref.numel():
                continue
            scale = max(1.0, ref.abs().max().item())
            if (generic64[name] - ref).abs().max().item() > 1e-12 * scale:
                problems.append(f"{c['desc']}: the generic restatement differs from the suite's in {name}")
            own = (want32[name].double() - ref).abs().max().item()
            if not (own == own and own != float("inf")):
                problems.append(f"{c['desc']}: the float32 restatement of {name} is not finite")
            tol = fwd_tol if name in ("out", "att_loss") else grad_tol
            if FF.OWN_FACTOR * own > tol * scale:
                hit("ill-conditioned (the float32 restatement sets the bar)")
        if redraws:
            hit("data redrawn")
        dup = FF.duplicate_rows(c)
        if bool(dup.any()):
            hit("cotangent zeroed on a row of 256 or more copies of one edge")
            if float(data["cot"][dup].abs().max()) != 0.0:
                problems.append(f"{c['desc']}: the cotangent of the duplicate rows")
        if kind in FF.ATTENTION:
            for cls in layout_classes(c):
                hit(cls)
        fwd, bwd = FF.row_lengths(c["ei"], n, c["mode"])
        for cls in row_classes(fwd):
            hit("forward row of " + cls)
        for cls in row_classes(bwd):
            hit("transposed row of " + cls)
        if n <= 3:
            hit(f"n = {n}")
        for opt, val in option_values(c):
            hit(f"{opt} = {val}")
    return table, problems


def test_every_pinned_case_is_well_posed_and_its_float32_yardstick_finite():
    _, problems = replay()
    assert not problems, "\n".join(problems)


def test_pinned_seeds_reach_every_class_for_every_kind():
    table, _ = replay()
    missing = []
    for kind in FF.KINDS:
        need = []
        if kind in FF.ATTENTION:
            need += [cls for cls in LAYOUT_CLASSES if cls not in NOT_FOR.get(kind, ())]
        for side in ("forward", "transposed"):
            need += [f"{side} row of {cls}" for cls in ROW_CLASSES if cls != "0" or FF.LOOPS[kind] == FF.LOOPS_KEEP]
        need += [f"n = {n}" for n in (1, 2, 3)]
        if kind in FF.SOFTMAX:
            need += ["cotangent zeroed on a row of 256 or more copies of one edge"]
        need += [f"{opt} = {val}" for opt, val in sorted(required_options(kind), key=str)]
        print(f"\n{kind}: {len(FF.pinned_seeds()) // len(FF.KINDS)} pinned cases")
        for cls in need + sorted(set(table[kind]) - set(need)):
            seeds = table[kind].get(cls, [])
            print(f"  {cls:58s} {len(seeds):3d}  {seeds[:6]}")
            if not seeds:
                missing.append((kind, cls))
    assert not missing, missing


def test_a_misaligned_operand_is_copied_before_a_wide_head_stops_fitting_a_wave():
    """What the fuzz's offset views found. pick_vec lowers the vector width to what the operands' pointers allow, and
    make_layout refuses a head that then needs more than 64 lanes, although *_supported takes the width: the library's
    host-side check returns RGBX_E_SHAPE for C = 128 behind a pointer 4 bytes off the grid. ops._rows_on_grid is what the
    ops put in front of it: views on the grid stay views, anything else is copied once into an aligned matrix."""
    from rgb_experiment_amd import _lib, ops
    lib = _lib.load()
    # 16-byte aligned, non-null, never dereferenced: the calls below return before a launch BECAUSE the library refuses
    # them. This pins a limitation of pick_vec / make_layout, not a contract: should they learn to take a wide head at a
    # lowered vector width, these calls would go on to a launch with made-up addresses and must be taken out first
    p = 0x10000

    def fwd(xl, C):
        return lib.rgbx_gatv2_fwd_f32(p, p, xl, C, p, C, p, None, p, C, p, p, 10, 1, C, 0.2, None, 0.0, None, None)
    assert lib.rgbx_gatv2_supported(1, 128) and lib.rgbx_gatv2_supported(1, 256)
    assert fwd(p + 4, 128) == -5 and b"lanes per head" in lib.rgbx_last_error_string()
    assert fwd(p + 8, 256) == -5 and b"lanes per head" in lib.rgbx_last_error_string()
    assert [ops._head_vec(C) for C in (1, 64, 66, 128, 132, 256)] == [1, 1, 2, 2, 4, 4] == \
        [FF.min_vec(C) for C in (1, 64, 66, 128, 132, 256)]
    flat = torch.zeros(4 * 8 + 4)
    fresh, offset = flat[:32].view(4, 8), flat[1:33].view(4, 8)
    block, odd_block = torch.zeros(4, 16)[:, 8:], torch.zeros(4, 11)[:, 3:]
    assert offset.is_contiguous() and offset.contiguous() is offset and offset.data_ptr() % 16 == 4
    assert ops._rows_on_grid(fresh) is fresh and ops._rows_on_grid(block) is block
    for t in (offset, odd_block, torch.zeros(8, 4).t()):
        got = ops._rows_on_grid(t)
        assert got is not t and torch.equal(got, t) and got.is_contiguous() and got.data_ptr() % 16 == 0
    assert ops._rows_on_grid(offset, 1) is offset and ops._rows_on_grid(odd_block, 1) is odd_block
    one_row = torch.zeros(1, 16)[:, 3:11]
    assert one_row.is_contiguous() and ops._rows_on_grid(one_row) is not one_row


def test_duplicate_rows_are_found_from_the_graph_alone():
    """Seed 4168's hub row (1024 copies of one edge and the self-loop) is one; its row of 62 copies is not; no other family
    has such rows; a row of DUP_LIMIT - 1 copies is none."""
    c = FF.draw_case(4168)
    assert c["kind"] == "gatv2" and FF.duplicate_rows(c).tolist() == [False, True]
    data, _, _ = FF.posed_data(c)
    assert float(data["cot"][1].abs().max()) == 0.0 and float(data["cot"][0].abs().min()) > 0.0
    assert not bool(FF.duplicate_rows(FF.draw_case(2291)).any())  # faconv: the kernel was mended instead
    ei = torch.stack([torch.zeros(FF.DUP_LIMIT - 1, dtype=torch.int64), torch.ones(FF.DUP_LIMIT - 1, dtype=torch.int64)])
    toy = {"kind": "transformer", "n": 2, "mode": FF.LOOPS_KEEP, "ei": ei}
    assert not bool(FF.duplicate_rows(toy).any())
    toy["ei"] = torch.cat([ei, ei[:, :1]], dim=1)
    assert FF.duplicate_rows(toy).tolist() == [False, True]


def test_parameters_off_the_grid_are_copied_too():
    """pick_vec counts the pointers of att, att_l, att_r and bias as well: a contiguous slice of a flat parameter buffer
    keeps its pointer through .reshape().contiguous(); ops._vec_on_grid copies it, and leaves one on the grid alone."""
    from rgb_experiment_amd import ops
    flat = torch.arange(40, dtype=torch.float32)
    off, on = flat[1:33].view(1, 4, 8), flat[4:36].view(1, 4, 8)
    assert off.reshape(32).contiguous().data_ptr() % 16 == 4
    got = ops._vec_on_grid(off, 32)
    assert got.data_ptr() % 16 == 0 and got.shape == (32,) and torch.equal(got, flat[1:33])
    assert ops._vec_on_grid(on, 32).data_ptr() == on.data_ptr() and ops._vec_on_grid(None, 32) is None
    assert not ops._vec_on_grid(off.clone().requires_grad_(True), 32).requires_grad
