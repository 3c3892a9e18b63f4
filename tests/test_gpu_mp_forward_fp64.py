"""The GATv2 message-passing forward against float64 on every kernel path: the node-chunk kernel (csrc/isg_mp.hip), the grouped and
the flat per-graph kernel (csrc/isg_mp_graph.hip), in every result form -- fp32 rows, rows with row maxima, segmented planes32, half
rows, and the four entry points that take the attention logits from the caller.

Reference: tests/mp_forward_restated.py (oracle.model.gatv2_message_passing plus bias) in float64 on the CPU.  Yardstick: the SAME
formula in float32.  For `out` and `alpha` of every run

    e_k  = max |kernel - ref64| / max |ref64|          e_32 = max |formula32 - ref64| / max |ref64|

and the test asserts  e_k <= max(F * e_32, FLOOR), FLOOR = 2e-6 (the project's floor).  No comparison may be decided by a bound
F * e_32 above CAP = 1e-3 (tests/test_mp_forward_cases_cpu.py asserts 8 * e_32 <= CAP for the formula alone, without a GPU).  alpha
also obeys the bound per element of tests/test_gpu_graph_tail_fp64.py: |alpha - alpha64| <= alpha64 * (expm1(2 F e_l) + 1e-5) + 3e-6
with e_l the float32 formula's own largest logit error in that destination and head.  Half rows: the formula in float64 on the
half-rounded rows, `out` within the half step of test_gatv2_message_passing_fp16_rows_match_oracle, alpha by the fp32 rule.  Logits
handed in: the float64 formula's logits rounded to float32, permuted into CSR slot order; reference and yardstick start from the same
float32 logits (softmax with + 1e-16, alpha * mask, aggregation), so nothing hides behind the edge-logits GEMM's tolerance.

Which kernel and instantiation a case launches is not taken on trust: mp_forward_restated.route() restates the dispatch under the
default environment (the fixture refuses a run with one of ISG_MP_LDS_KB, ISG_MPF_LDS_KB, ISG_MP_FLAGS, ISG_MP_FORCE_GRAPH,
ISG_MP_NO_FLAT set) and tests/test_mp_forward_cases_cpu.py proves, on the host, that every case reaches the branch it names and that
the cases together launch all 118 instantiations any supported input reaches; the other 48 are UNREACHABLE there, by name.

Cases (92; topologies of at most 285 nodes and 1200 edges, edge order shuffled, duplicate edges, self loops on all but chosen nodes):
  node-chunk   all 32 (H, P) on "small" (1-node graphs, an empty graph in the middle, trailing ones, a 40-edge hub: beyond MP_LCAP),
               the last pass full and partly filled; N = 16 and 17 as whole batches; E = 0; "hub": 1164 slots in the first 16-node
               block, the hub's segment across slot 1024; and what leaves the per-graph kernels with kernel="graph": 257 nodes, 1025
               slots, the 8-row floor of the large tables (H = 8; H = 4 at C = 72), P = 3, the flat rule beyond 64 nodes
  grouped      every reachable (HS, P, exact) on the small tables (13) and the large ones (8: "t65", one node past the small tables);
               H = 3 and 16; Q = 90 just past the flat rule; 64 nodes / 256 slots; 257 slots; 256 nodes / 1024 slots; windows of 33
               rows (H, C = 4, 128, small tables) and 14 rows (large tables) with graphs of lrows and lrows + 1 nodes, the last node a
               source; N = 16, 17; E = 0
  flat         C = 260, 268, 300, 356 (both ends of the rule), H = 2, 4, 8; 64 nodes / 256 slots; the 14-row window at 14 / 15 nodes
Classes: plain; sharp (att x 8, |logit| up to 49); shift (every logit near + 32, through x_r along sign(att)); mask01 (0/1 node mask,
0.99999994 on some picked nodes); edge01; frac (fractional_mask on the edges: -0.0, values above 1); dead (one destination with
every in-edge masked, one graph masked completely: alpha uniform, out == bias); far (shift at + 100, added to the issue's list: at
+ 32 a softmax without `- mx` is still right to 1e-6, exp(100) is not a float32).
Forms, per case and class: rows with dense operands, with x_l | x_r as column slices of one [N, 2 H C] tensor and e_proj a slice of
[E, 3 H C] (the same bits), twice (the same bits); want_rowmax (the same rows, maxima bit-equal to out.view(N, H, C).abs().amax(2); no
maxima and the same rows where the flat or the node-chunk kernel runs); want_planes at H = 4 (planes and scales bit-equal to
isg_split_planes32 of each half of the rows on flat widths, the rows elsewhere); half rows (IsgError where route() has no kernel);
isg_gatv2_mp_fwd_logits with and without rowmax, _logits_f16, _logits_planes through the library handle (ISG_EUNSUPPORTED exactly
where route() says so).  Exact: out == bias bit for bit where nothing is aggregated (no in-edge, every in-edge masked, a masked
destination, E = 0), alpha == 1.0 on a single in-edge, alpha rows of unmasked runs sum to 1 within 1e-5, alpha uniform on the dead
destination.  test_what_has_no_kernel_is_refused_on_the_host: C % 4, H = 3 and nine passes on the node-chunk kernel, half rows
wherever the grouped kernel does not run.

Measured on the MI355X from this tree with F = 8 (per kernel family and class, `out` and `alpha` together; "above the floor" = the
comparisons with e_k > FLOOR, where F decides, and their largest e_k / e_32; "logits in" = the four entry points that take logits;
the same figures go through conftest.parity_record, and test_zz_the_table_of_this_run prints them):

    family             class                  comparisons  max e_k   e_32 range          max ratio   above the floor
    chunk              plain, dead            95 + 94      2.5e-7    0 .. 2.3e-7         2.28        --
    chunk              mask01, edge01, frac   95 + 94 + 94 1.4e-6    0 .. 1.6e-6         2.44        --
    chunk              sharp                  94           1.4e-6    1.7e-7 .. 1.4e-6    2.92        --
    chunk              shift                  94           1.6e-6    1.8e-7 .. 2.2e-6    1.46        --
    chunk              far                    94           5.4e-6    5.0e-7 .. 5.9e-6    1.47        1.30 (36 comparisons)
    grouped            plain, dead            69 + 68      1.6e-7    0 .. 1.7e-7         1.94        --
    grouped            mask01, edge01, frac   69 + 68 + 68 3.2e-7    0 .. 3.5e-7         2.00        --
    grouped            sharp                  68           1.5e-6    1.7e-7 .. 1.5e-6    1.95        --
    grouped            shift                  68           2.0e-6    2.2e-7 .. 2.0e-6    1.42        --
    grouped            far                    68           4.7e-6    7.3e-7 .. 5.9e-6    1.13        1.08 (32)
    grouped f16 alpha  all but far            7 x 34       1.9e-6    5.5e-8 .. 1.8e-6    2.12        --
    grouped f16 alpha  far                    34           5.3e-6    2.8e-6 .. 6.1e-6    1.28        1.28 (34)
    flat               all but far            114          1.6e-6    0 .. 1.6e-6         1.76        --
    flat               far                    16           4.5e-6    8.1e-7 .. 5.4e-6    1.20        1.20 (8)
    grouped logits in  all eight              8 x 136      3.1e-7    2.5e-8 .. 3.0e-7    2.13        --
    grouped logits f16 all eight (alpha)      8 x 34       4.7e-7    2.5e-8 .. 4.7e-7    1.97        --
    flat logits in     all eight              8 x 22       2.9e-7    3.2e-8 .. 2.9e-7    1.78        --

alpha per element, of its bound at F = 8: 0.44 at most (chunk, far; 0.34 grouped f16, 0.21 grouped and flat, far; 0.19 under shift,
0.11 elsewhere; 0.05 at most with the logits handed in).  Half rows: `out` within 0.997 of the half step in all 8 x 35 + 8 x 34
comparisons (a rounding the other way is one step, which is the bound).
F = 4.  Only the far class has comparisons above the floor (110 of 3238); their largest ratio is 1.30 (node-chunk kernel), and 4 is
the smallest of 2, 4, 8 that leaves a factor of 2 over it.  The per-element figures can double at most from F = 8 to 4 (the bound is
convex in F); run again with F = 4 the largest is 0.48 (chunk, far).  The largest bound that decides a comparison is 4 * 6.1e-6 = 2.4e-5, under the cap.  Below the floor the
largest ratio is 2.92 (hub, H = 1, C = 300, sharp, alpha: e_k = 1.2e-6 against 4.0e-7): one float32 rounding of a logit of size 49 is
3.8e-6 of the weight it belongs to, and kernel and formula round their 300-term logit sums in different orders; per element that
comparison sits at 0.09 of its bound.  The hardware exp / rcp of the per-graph kernels do not show: their ratios are below the
node-chunk kernel's expf and division in every class.
No comparison failed on the first run and no bit-for-bit or exact expectation did: this work found no defect in the kernels, and csrc/
is unchanged.  What it did find is on the host side of the record: 48 instantiations are dead under the default environment (grouped
HS = 8 on the large tables, HS = 4 there at P = 2 and at the exact C = 64, EXACT at P = 2 unless HS = 1, the flat kernel's P = 2 and
P = 4: UNREACHABLE in tests/mp_forward_restated.py says why, DESIGN.md section 4 lists them), and a comment in MP_CASES of
tests/test_gpu_ops.py named the wrong kernel (corrected).

As a self-check the kernels were broken five ways on five scratch builds (nothing of it is in the tree), changing values but no address;
beside this file ran the 119 older GPU tests of test_gpu_ops.py named after message passing and the edge-logits pair:
  * no `- mx` in the grouped kernel's phase C: all 13 grouped tests with edges fail -- far in every case and form (not finite), sharp in
    8 to 10 of 34 cases (by the rule and per element), shift in none, which is why far exists.  Older tests: 3 of 26
    test_gatv2_message_passing_matches_oracle, 3 of 6 fp16, 1 planes case, and the edge-logits pair's;
  * a source row beyond the window read from LDS row 0: the 7 tests with a graph larger than its window fail (grouped-L-*, e257, t256,
    t64, win), in every class, and no test without one.  Older tests: 4 of 26 test_gatv2_message_passing_matches_oracle (the MP_CASES with 50 to 70 nodes), 2 fp16, the pair's;
  * the last channel pass without its bias: all 14 grouped tests fail, in every class and form, by the rule and by out == bias.  Older
    tests: 11 of 26 and all 6 fp16 cases, the pair's;
  * rowmax written before the bias: all 13 grouped tests with edges fail, in the row-maxima comparisons only (want_rowmax and
    logits_rowmax, every class).  None of the older message-passing tests fails; 28 of the edge-logits pair's and the tile convolution's do;
  * one pass left out at P = 3 in the node-chunk kernel: chunk-H1, -H2, -H4, -H8 and chunk-behind-graph (H = 1, C = 516) fail, at
    the P = 3 widths only, in `out` of every class.  All 119 older tests pass.
"""
import os

import pytest
import torch

import mp_forward_restated as R
from conftest import parity_record
from test_gpu_graph_tail_fp64 import errors

FLOOR = 2e-6
F = 4
CAP = 1e-3
F32, F16 = torch.float32, torch.float16
STATS = {}          # (family, class) -> [comparisons, max e_k, min e_32, max e_32, max ratio, max ratio above the floor, those above it]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    set_ = [k for k in R.ENV_SWITCHES if k in os.environ]
    assert not set_, f"route() restates the dispatch under the default environment; unset {set_}"
    return torch.device("cuda:0")


# ---- the rule -------------------------------------------------------------------------------------------------------------
class Judge:
    """Collects every comparison of one test; prints each figure before anything is asserted, and puts them on record."""

    def __init__(self, name):
        self.name, self.bad, self.rows, self.case = name, [], {}, ""

    def __call__(self, family, cls, what, got, ref64, ref32):
        name = f"{self.case} | {family} | {cls} | {what}"
        got = got.detach().cpu()
        if tuple(got.shape) != tuple(ref64.shape):
            self.bad.append(f"{name}: shape {tuple(got.shape)}, reference {tuple(ref64.shape)}")
            return
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{name}: not finite")
            return
        e_k, e_32, zero = errors(got, ref64, ref32)
        if e_k is None:                           # an empty tensor, or a reference that is zero everywhere: exact zeros
            if zero:
                self.bad.append(f"{name}: the reference is zero there, the kernel has {zero:.3e}")
            return
        bound = max(F * e_32, FLOOR)
        ratio = e_k / max(e_32, 1e-30)
        print(f"[fp64] {name} | e_k={e_k:.3e} e_32={e_32:.3e} ratio={ratio:.2f}")
        self.rows[name] = {"e_k": e_k, "e_32": e_32}
        s = STATS.setdefault((family, cls), [0, 0.0, float("inf"), 0.0, 0.0, 0.0, 0])
        above = e_k > FLOOR
        s[:] = [s[0] + 1, max(s[1], e_k), min(s[2], e_32), max(s[3], e_32), max(s[4], ratio if e_32 > 0 else 0.0),
                max(s[5], ratio if above else 0.0), s[6] + above]
        if F * e_32 > CAP:
            self.bad.append(f"{name}: ill-posed case, F * e_32 = {F * e_32:.3e} > {CAP:.0e}")
        if not e_k <= bound:
            self.bad.append(f"{name}: e_k = {e_k:.3e} > max({F} * e_32, floor) = {bound:.3e}  (e_32 = {e_32:.3e})")

    def alpha_elem(self, family, cls, what, got, ei, N, r64, r32):
        """The bound per element of tests/test_gpu_graph_tail_fp64.py on a softmax weight: |alpha - alpha64| <= alpha64 *
        (expm1(2 F e_l) + 1e-5) + 3e-6, e_l the float32 formula's own largest logit error in that destination and head."""
        name = f"{self.case} | {family} | {cls} | {what} per element"
        H = r64["alpha"].size(1)
        if r64["alpha"].numel() == 0:
            return
        seg = (ei[1][:, None] * H + torch.arange(H)[None, :]).reshape(-1)
        e_l = torch.zeros(N * H, dtype=torch.float64).scatter_reduce_(0, seg, (r32["logits"].double() - r64["logits"]).abs().reshape(-1), "amax")
        a64 = r64["alpha"].reshape(-1)
        lim = a64 * (torch.expm1(2.0 * F * e_l[seg]) + 1e-5) + 3e-6
        rel = float(((got.detach().cpu().reshape(-1).double() - a64).abs() / lim).max())
        print(f"[fp64] {name} | {rel:.3f} of its bound (largest logit error of the float32 formula {float(e_l.max()):.2e})")
        self.rows[name] = {"of_bound": rel}
        s = STATS.setdefault((family, cls + " alpha/elem"), [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0])
        s[0], s[1] = s[0] + 1, max(s[1], rel)
        if not rel <= 1.0:
            self.bad.append(f"{name}: {rel:.3f} of the bound")

    def half_rows(self, family, cls, what, got, ref64):
        """The half-ulp rule of test_gatv2_message_passing_fp16_rows_match_oracle: one half step at |ref| plus 4e-6."""
        name = f"{self.case} | {family} | {cls} | {what}"
        got, ref = got.detach().cpu().float(), ref64.half().float()
        if tuple(got.shape) != tuple(ref.shape) or not bool(torch.isfinite(got).all()):
            self.bad.append(f"{name}: shape or not finite")
            return
        ulp = torch.maximum(ref.abs(), torch.tensor(6.1e-5)) * 2.0 ** -10 + 4e-6
        rel = float(((got - ref).abs() / ulp).max()) if got.numel() else 0.0
        other = float((got != ref).float().mean()) if got.numel() else 0.0
        print(f"[fp64] {name} | {rel:.3f} of a half step, {other:.4f} of the entries rounded the other way")
        self.rows[name] = {"of_half_step": rel, "other_rounding": other}
        s = STATS.setdefault((family, cls + " half out"), [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0])
        s[0], s[1] = s[0] + 1, max(s[1], rel)
        if not rel <= 1.0:
            self.bad.append(f"{name}: {rel:.3f} of a half step")

    def same_bits(self, name, a, b):
        a, b = a.detach().cpu(), b.detach().cpu()
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape) or not torch.equal(a, b):
            far = float((a.double() - b.double()).abs().max()) if tuple(a.shape) == tuple(b.shape) and a.numel() else float("nan")
            self.bad.append(f"{self.case} | {name}: not the same bits (max distance {far:.3e})")

    def check(self, ok, text):
        if not ok:
            self.bad.append(f"{self.case} | {text}")

    def done(self):
        parity_record(f"mp_forward_fp64 {self.name}", self.rows)
        assert not self.bad, f"{self.name}:\n  " + "\n  ".join(self.bad)


# ---- operands and calls ---------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_of(topo, dev):
    from isubgvqa_amd import ops
    if topo not in _PLANS:
        batch, ei, sizes = R.topology(topo)
        plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=len(sizes))
        c = R.csr(topo)
        assert (plan.nmax, plan.emax, plan.B, plan.N, plan.E) == (c["nmax"], c["emax"], c["B"], c["N"], c["E"]), topo
        assert torch.equal(plan.eid[:c["E"]].cpu().long(), c["eid"]), topo
        _PLANS[topo] = plan
    return _PLANS[topo]


def on_dev(t, dev, half=False):
    d = {k: None if v is None else v.to(dev) for k, v in t.items()}
    if half:
        for k in ("x_l", "x_r", "e_proj"):
            d[k] = d[k].half()
    return d


def strided(d):
    """x_l | x_r as the column halves of one [N, 2 H C] tensor, e_proj as the middle third of an [E, 3 H C] one."""
    HC = d["x_l"].size(1)
    xlr = torch.cat([d["x_l"], d["x_r"]], 1)
    e3 = torch.cat([d["e_proj"] + 1.0, d["e_proj"], d["e_proj"] - 1.0], 1)
    s = dict(d, x_l=xlr[:, :HC], x_r=xlr[:, HC:], e_proj=e3[:, HC:2 * HC])
    assert s["x_l"].stride(0) == 2 * HC and s["e_proj"].stride(0) == 3 * HC
    return s


def mp(d, plan, H, kernel, **kw):
    from isubgvqa_amd import ops
    with torch.no_grad():
        return ops.gatv2_mp(d["x_l"], d["x_r"], d["e_proj"], d["att"], plan, H, bias=d["bias"], node_mask=d["node_mask"],
                            edge_mask=d["edge_mask"], negative_slope=R.SLOPE, kernel=kernel, **kw)


def mp_logits(form, d, logits_slot, plan, H, C):
    """isg_gatv2_mp_fwd_logits (form "logits" / "logits_rowmax"), _logits_f16 (half rows) and _logits_planes through the library
    handle, in the argument order of ops.gatv2_mp_edge_logits: (status, out or Planes32, alpha, rowmax or None)."""
    from isubgvqa_amd import _lib, ops
    lib = _lib.load()
    x_l = d["x_l"]
    N, HC = x_l.shape
    E = plan.E
    attp, biasp, nm, em = ops._mp_operands(d["att"], d["bias"], d["node_mask"], d["edge_mask"], N, E, HC)
    alpha = torch.full((E, H), float("nan"), dtype=F32, device=x_l.device)
    ins = (x_l.data_ptr(), logits_slot.data_ptr(), attp, biasp, plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), nm, em)
    dims = (N, E, H, C, R.SLOPE, plan.ptr.data_ptr(), plan.eptr.data_ptr(), plan.dst.data_ptr(), plan.B, plan.nmax, plan.emax,
            x_l.stride(0), ops._stream())
    if form == "logits_planes":
        planes, pl, pinv = ops._segmented_planes32(N, H, C, x_l.device)
        return lib.isg_gatv2_mp_fwd_logits_planes(*ins, pl, pinv, alpha.data_ptr(), *dims), planes, alpha, None
    out = torch.full((N, HC), float("nan"), dtype=x_l.dtype, device=x_l.device)
    if x_l.dtype == F16:
        return lib.isg_gatv2_mp_fwd_logits_f16(*ins, out.data_ptr(), alpha.data_ptr(), *dims), out, alpha, None
    rowmax = torch.full((N, H), float("nan"), dtype=F32, device=x_l.device) if form == "logits_rowmax" else None
    rc = lib.isg_gatv2_mp_fwd_logits(*ins, out.data_ptr(), alpha.data_ptr(), 0 if rowmax is None else rowmax.data_ptr(), *dims)
    return rc, out, alpha, rowmax


def planes_match(judge, what, got, rows, C):
    """The segmented planes32 result against isg_split_planes32 of each half of the fp32 rows, as
    test_message_passing_result_as_segmented_planes states it."""
    from isubgvqa_amd import ops
    N = rows.size(0)
    judge.check(isinstance(got, ops.Planes32) and got.seg_cols == 2 * C and got.rows == N and got.cols == 4 * C, f"{what}: not a segmented Planes32")
    if not isinstance(got, ops.Planes32):
        return
    st = (2 * C + 31) // 32
    for half, inv in ((0, got.inv_first), (1, got.inv)):
        ref = ops.split_planes32(rows[:, half * 2 * C:(half + 1) * 2 * C].contiguous())
        mine = got.planes.view(N, 2 * st, 64)[:, half * st:(half + 1) * st].contiguous().view(-1)
        judge.same_bits(f"{what}: inverse scales of half {half}", inv, ref.inv)
        judge.same_bits(f"{what}: planes of half {half}", mine, ref.planes)


def exact_expectations(judge, what, case, cls, out, alpha, t, half=False):
    """What the formula gives exactly: out == bias where nothing is aggregated, alpha == 1 on a single in-edge, rows of alpha that
    sum to one, equal weights where every logit is the same zero."""
    _, ei, _ = R.topology(case.topo)
    c = R.csr(case.topo)
    out, alpha = out.detach().cpu(), alpha.detach().cpu()
    idle = c["deg"] == 0
    if cls == "mask01":
        idle = idle | (t["node_mask"].reshape(-1) == 0)
    if cls == "dead":
        live = torch.zeros(c["N"], dtype=torch.long).index_add_(0, ei[1], (t["edge_mask"].reshape(-1) != 0).long())
        idle = idle | (live == 0)
        node, graph = R.dead_parts(case.topo)
        judge.check(bool(idle[node]) and (graph is None or bool(idle[c["ptr"][graph]:c["ptr"][graph + 1]].all())), f"{what}: the dead parts are not dead")
        a = alpha[ei[1] == node]
        judge.check(bool((a == a[0]).all()), f"{what}: alpha of the fully masked destination is not uniform")
    bias = t["bias"].half() if half else t["bias"]
    judge.check(bool(idle.any()) or c["N"] <= 17, f"{what}: no destination without a live in-edge")
    judge.same_bits(f"{what}: out == bias where nothing is aggregated", out[idle], bias.expand(c["N"], -1)[idle])
    if c["E"] == 0:
        return
    single = (c["deg"] == 1)[ei[1]]
    judge.check(bool((alpha[single] == 1.0).all()), f"{what}: alpha of a single in-edge is not exactly 1")
    if R.MASK_OF[cls] is None:
        s = torch.zeros(c["N"], alpha.size(1)).index_add_(0, ei[1], alpha)[c["deg"] > 0]
        judge.check(bool(((s - 1.0).abs() <= 1e-5).all()), f"{what}: alpha rows do not sum to one ({float((s - 1).abs().max()):.2e})")


# ---- one case, every class and every form --------------------------------------------------------------------------------
def run_case(judge, case, dev):
    from isubgvqa_amd import _lib, ops
    topo, H, C, kernel = case.topo, case.H, case.C, case.kernel
    judge.case = case.id
    _, ei, _ = R.topology(topo)
    c = R.csr(topo)
    N, E = c["N"], c["E"]
    plan = plan_of(topo, dev)
    key = (topo, H, C)
    for cls in R.classes_of(topo):
        masked = R.MASK_OF[cls] is not None
        rt = lambda form, dt=F32: R.case_route(case, form, dt, masked)
        fam = rt("rows")[0]
        assert fam == case.family
        t = R.inputs(*key, cls)
        d = on_dev(t, dev)
        r64, r32 = R.reference(*key, cls, torch.float64), R.reference(*key, cls, F32)

        # rows: dense, strided, twice
        out, alpha = mp(d, plan, H, kernel)
        judge(fam, cls, "rows out", out, r64["out"], r32["out"])
        judge(fam, cls, "rows alpha", alpha, r64["alpha"], r32["alpha"])
        judge.alpha_elem(fam, cls, "rows alpha", alpha, ei, N, r64, r32)
        exact_expectations(judge, f"{cls} rows", case, cls, out, alpha, t)
        o2, a2 = mp(strided(d), plan, H, kernel)
        judge.same_bits(f"{cls}: out, strided operands", o2, out)
        judge.same_bits(f"{cls}: alpha, strided operands", a2, alpha)
        o3, a3 = mp(d, plan, H, kernel)
        judge.same_bits(f"{cls}: out, second call", o3, out)
        judge.same_bits(f"{cls}: alpha, second call", a3, alpha)
        if kernel == "chunk":
            continue

        # row maxima: the same rows, and the maxima of exactly those rows -- or rows without maxima
        o, a = mp(d, plan, H, kernel, want_rowmax=True)
        judge.same_bits(f"{cls}: out with want_rowmax", o, out)
        judge.same_bits(f"{cls}: alpha with want_rowmax", a, alpha)
        if rt("rowmax") != "unsupported" and E > 0:
            judge.check(ops.row_maxima(o) is not None, f"{cls}: no row maxima where {rt('rowmax')} has them")
            if ops.row_maxima(o) is not None:
                judge.same_bits(f"{cls}: row maxima", ops.row_maxima(o), out.view(N, H, C).abs().amax(2))
        else:
            judge.check(ops.row_maxima(o) is None, f"{cls}: row maxima from a kernel that has none")

        # planes (H = 4): the flat kernel's segmented planes32, or the rows
        if H == 4:
            p, a = mp(d, plan, H, kernel, want_planes=True)
            judge.same_bits(f"{cls}: alpha with want_planes", a, alpha)
            if rt("planes") != "unsupported" and E > 0:
                planes_match(judge, f"{cls} planes", p, out, C)
            else:
                judge.check(isinstance(p, torch.Tensor), f"{cls}: planes from a kernel that has none")
                if isinstance(p, torch.Tensor):
                    judge.same_bits(f"{cls}: rows with want_planes", p, out)

        # half rows: the formula in float64 on the half-rounded rows
        dh = on_dev(t, dev, half=True)
        r64h, r32h = R.reference(*key, cls, torch.float64, True), R.reference(*key, cls, F32, True)
        if rt("rows", F16) != "unsupported":
            oh, ah = mp(dh, plan, H, kernel)
            judge.check(oh.dtype == F16 and ah.dtype == F32, f"{cls}: half rows came back as {oh.dtype}")
            judge.half_rows(fam, cls, "half rows out", oh, r64h["out"])
            judge(fam + " f16", cls, "half rows alpha", ah, r64h["alpha"], r32h["alpha"])
            judge.alpha_elem(fam + " f16", cls, "half rows alpha", ah, ei, N, r64h, r32h)
            exact_expectations(judge, f"{cls} half rows", case, cls, oh, ah, t, half=True)
        else:
            with pytest.raises(_lib.IsgError):
                mp(dh, plan, H, kernel)

        # logits handed in: the float64 formula's, rounded to float32, in CSR slot order
        if E == 0:
            continue
        for form, half in (("logits", False), ("logits_rowmax", False), ("logits", True), ("logits_planes", False)):
            if form == "logits_planes" and H != 4:
                continue
            lg, l64 = R.reference_from_logits(*key, cls, torch.float64, half)
            _, l32 = R.reference_from_logits(*key, cls, F32, half)
            slot = lg[c["eid"]].contiguous().to(dev)
            rc, o, a, rmx = mp_logits(form, dh if half else d, slot, plan, H, C)
            want = rt(form, F16 if half else F32)
            tag = f"{form}{' f16' if half else ''}"
            if want == "unsupported":
                judge.check(rc == ops.ISG_EUNSUPPORTED, f"{cls} {tag}: status {rc} where route() says unsupported")
                continue
            judge.check(rc == 0, f"{cls} {tag}: status {rc} where route() says {want}")
            if rc != 0:
                continue
            lfam = f"{want[0]} logits in" + (" f16" if half else "")
            judge(lfam, cls, f"{tag} alpha", a, l64["alpha"], l32["alpha"])
            judge.alpha_elem(lfam, cls, f"{tag} alpha", a, ei, N, l64, l32)
            if form == "logits_planes":
                rows = mp_logits("logits", d, slot, plan, H, C)[1]
                planes_match(judge, f"{cls} {tag}", o, rows, C)
                continue
            if half:
                judge.half_rows(lfam, cls, f"{tag} out", o, l64["out"])
            else:
                judge(lfam, cls, f"{tag} out", o, l64["out"], l32["out"])
            exact_expectations(judge, f"{cls} {tag}", case, cls, o, a, t, half=half)
            if rmx is not None:
                judge.same_bits(f"{cls} {tag}: row maxima", rmx, o.view(N, H, C).abs().amax(2))
                rows = mp_logits("logits", d, slot, plan, H, C)
                judge.same_bits(f"{cls} {tag}: out with and without row maxima", o, rows[1])
                judge.same_bits(f"{cls} {tag}: alpha with and without row maxima", a, rows[2])


def _groups():
    g = {}
    for case in R.CASES:
        if case.family == "chunk":
            name = f"chunk-H{case.H}" if case.topo == "small" and case.kernel == "chunk" and case.want[1] == case.H and case.C != 300 \
                else ("chunk-edges" if case.kernel == "chunk" else "chunk-behind-graph")
        elif case.family == "grouped":
            name = f"grouped-{case.want[4]}-HS{case.want[1]}" if case.topo in ("small", "t65") else f"grouped-edges-{case.topo}"
        else:
            name = "flat-small" if case.topo == "small" else "flat-edges"
        g.setdefault(name, []).append(case)
    return g


GROUPS = _groups()


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_mp_forward_against_fp64(dev, group):
    """Every case of a kernel family and width group, every class, every form route() names for it: by the rule, bit for bit where
    two forms must agree, exactly where the formula is exact, the documented fallback where a form does not exist."""
    judge = Judge(group)
    for case in GROUPS[group]:
        run_case(judge, case, dev)
    judge.done()


REFUSED = [("C % 4 != 0", 4, 6, "graph", F32), ("C % 4 != 0, node-chunk", 4, 6, "chunk", F32), ("H = 3 on the node-chunk kernel", 3, 8, "chunk", F32),
           ("half rows on the node-chunk kernel", 4, 8, "chunk", F16), ("nine passes at H = 1", 1, 2052, "graph", F32),
           ("nine passes at H = 8", 8, 260, "chunk", F32), ("H = 3 at a flat width", 3, 300, "graph", F32),
           ("half rows at a flat width", 4, 300, "graph", F16), ("half rows behind the large tables' floor", 8, 16, "graph", F16)]


@pytest.mark.gpu
def test_what_has_no_kernel_is_refused_on_the_host(dev):
    """route() says "unsupported": the call raises before any launch (the result tensors are never written)."""
    from isubgvqa_amd import _lib
    for what, H, C, kernel, dt in REFUSED:
        topo = "t65" if "large tables" in what else "small"
        c = R.csr(topo)
        assert R.route(H, C, c["nmax"], c["emax"], c["B"], dt, "rows", kernel, False) == "unsupported", what
        gen = torch.Generator().manual_seed(H * C)
        r = lambda *s: torch.randn(*s, generator=gen).to(dt).to(dev)
        d = {"x_l": r(c["N"], H * C), "x_r": r(c["N"], H * C), "e_proj": r(c["E"], H * C), "att": torch.randn(1, H, C, generator=gen).to(dev),
             "bias": None, "node_mask": None, "edge_mask": None}
        with pytest.raises(_lib.IsgError):
            mp(d, plan_of(topo, dev), H, kernel)
        print(f"[fp64] refused: {what} (H = {H}, C = {C}, kernel = {kernel})")


@pytest.mark.gpu
def test_zz_the_table_of_this_run(dev):
    """Per kernel family and class, over whatever ran before in this process: comparisons, largest e_k, range of e_32, largest ratio,
    largest ratio among the comparisons above the floor (where F decides).  Always passes; the figures go on record."""
    table = {}
    print("[fp64] family | class | comparisons | max e_k | e_32 range | max ratio | max ratio above the floor (comparisons)")
    for (fam, cls), s in sorted(STATS.items()):
        if cls.endswith("alpha/elem") or cls.endswith("half out"):
            print(f"[fp64] {fam} | {cls} | {s[0]} | {s[1]:.3f} of the bound at most")
            table[f"{fam} | {cls}"] = {"comparisons": s[0], "of_bound": s[1]}
            continue
        print(f"[fp64] {fam} | {cls} | {s[0]} | {s[1]:.1e} | {s[2]:.1e} .. {s[3]:.1e} | {s[4]:.2f} | {s[5]:.2f} ({s[6]})")
        table[f"{fam} | {cls}"] = {"comparisons": s[0], "max_e_k": s[1], "e_32": [s[2], s[3]], "max_ratio": s[4], "max_ratio_above_floor": s[5],
                                   "above_floor": s[6]}
    parity_record("mp_forward_fp64 table", table)
