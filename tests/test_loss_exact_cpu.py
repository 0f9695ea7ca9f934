"""CPU: the exact-arithmetic fixtures of tests/ref_exact_loss.py without a GPU.

1. the preconditions of every fixture: the five terms are bf16-exact, the window sums times 256 are integers below 2^24, the
   denominator of the contrast map stays above 1/8, the L1 / L2 budgets; the operation counts K_PIXEL are what RE derives;
2. the tables reach what they claim to reach, from the dispatch arithmetic of the entry points (tiles per side, the last tile's
   extent, total % 8, VEC or not, the grid-stride loop of the pooling pass, the workgroups and slots of the stack maximum);
3. the plain-PyTorch entry points (ref_exact_loss.TorchEntry) pass the runners the GPU file runs on the library;
4. the statement agrees with the project's oracle: per-sample SSIM / CS means against oracle.loss_ref.ssim_25d within the 1e-3
   the project uses for this loss, the gradient fields against float64 autograd of the oracle's formula;
5. sensitivity: each seeded defect (ref_exact_loss.DEFECTS, one indexing error each) fails an exact runner; what the criteria of
   test_mixed_loss_vs_reference_golden (tests/test_gpu_model.py) make of the same defect on a (2, 2, 5, 192, 192) stack is recorded in
   OLD_TESTS_SEE and asserted, so the stated gap stays true: they see two of the six
   (both factor defects, and the sample mix-up only because this stack has B = 2)."""

import pytest
import torch

from oracle import loss_ref
from tests import ref_exact_loss as X

CPU = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()


def _ids(cases):
    return [c["name"] for c in cases]


def _case(name):
    return next(c for c in X.stack_cases() if c["name"] == name)


# ------------------------------------------------------------------------------------------------ 1. preconditions
@pytest.mark.parametrize("case", X.stack_cases(), ids=_ids(X.stack_cases()))
def test_stack_fixtures_are_within_the_exactness_budget(case):
    fx = X.stack_fixture(case)
    for same in (False, True):
        st = X.case_statement(case, same)
        # the running error bound divides by the denominator of the contrast map itself: this only keeps that factor below 8
        assert st["identity"] and st["sum_max"] < X.LIMIT and st["bd_min"] >= 0.125
        assert st["l1"] * 16 == round(st["l1"] * 16) < X.LIMIT and st["l2"] * 256 == round(st["l2"] * 256) < X.LIMIT
        assert torch.equal(st["Po"] * 64, (st["Po"] * 64).round()) and st["dr"] == float(fx["T"].max())
        for last in (0, 1):
            assert {k: st["fields"][last][k].k for k in X.K_PIXEL[last]} == X.K_PIXEL[last]
    k = fx["P"] * 16
    assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= 16
    same = X.case_statement(case, True)["fields"]   # P == T: every value of both maps is exactly 1
    assert all(torch.equal(same[l][m].v, torch.ones_like(same[l][m].v)) for l in (0, 1) for m in ("ssim", "cs"))


def test_chain_second_scale_is_within_its_budget():
    for case in X.chain_cases():
        st0 = X.case_statement(case)
        st1 = X.forward_statement(st0["Po"], st0["To"], q=12)   # asserts multiples of 2^-12 below 2^24 / 4096
        assert not st1["identity"] and st1["sum_max"] < X.LIMIT and case["H"] // 2 >= 11 and case["W"] // 2 >= 11


def test_running_error_rules():
    a, b = X.RE(torch.tensor([3.0, -5.0])), X.RE(torch.tensor([0.5, 7.0]))
    s = a * b - a                      # one product, one subtraction
    assert s.k == 2 and torch.equal(s.A, (a.v * b.v).abs() + a.v.abs())
    assert (X.RE(2.0) * a).k == 0 and (a + X.RE(0.0)) is a and (X.RE(0.0) * s).k == 0
    q = s / (a - b)
    assert q.k == 3 and bool((q.A >= q.v.abs()).all())


# ------------------------------------------------------------------------------------------------ 2. the tables
def test_stack_cases_reach_the_paths_they_are_listed_for():
    cases = X.stack_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    plan = {c["name"]: X.tile_plan(c["B"], c["C"], c["H"], c["W"], c["offset"]) for c in cases}
    for c in cases:
        p = plan[c["name"]]
        assert c["H"] >= 11 and c["W"] >= 11 and max(p["last_own"]) <= X.SI and min(p["last_out"]) >= 1
        assert f"= {p['fwd_total']} workgroups (total % 8 = {p['fwd_total'] % 8})" in c["leg"] and ("non-VEC" in c["leg"]) == (not p["vec"])
    p = plan["one_pixel_1x3x1x11x11"]
    assert p["fwd"] == (1, 1) and p["last_out"] == (1, 1) and p["fwd_total"] == 3 and p["fwd_total"] % 8 and p["bwd_total"] % 8
    p = plan["one_tile_1x1x5x42x42"]
    assert p["fwd"] == (1, 1) and p["last_out"] == (32, 32) and p["last_own"] == (42, 42) and p["bwd"] == (2, 2) and p["vec"]
    p = plan["edge_2x2x5x43x43"]
    assert p["fwd"] == (2, 2) and p["last_out"] == (1, 1) and p["last_own"] == (11, 11) and p["fwd_total"] == 16 and p["bwd_total"] == 16
    assert p["odd"] == (1, 1) and not p["vec"]
    p = plan["across_2x1x7x52x75"]
    assert p["fwd"] == (2, 3) and p["odd"] == (0, 1) and not p["vec"] and p["fwd_total"] == 12 and p["bwd_total"] == 12
    p, q = plan["vec_1x2x3x53x74"], plan["unaligned_1x2x3x53x74"]
    assert p["vec"] and not q["vec"] and p["odd"] == (1, 0) and p["fwd"] == q["fwd"] == (2, 2) and p["fwd_total"] % 8 == 0
    fa, fb = X.stack_fixture(_case("vec_1x2x3x53x74")), X.stack_fixture(_case("unaligned_1x2x3x53x74"))
    assert torch.equal(fa["P"], fb["P"]) and torch.equal(fa["T"], fb["T"])
    v = X.place(fa["P"], CPU, 1)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    p = plan["grids_1x2x3x65x33"]
    assert p["fwd"] == (2, 1) and p["bwd"] == (3, 2) and p["fwd_total"] % 8 and p["bwd_total"] % 8
    p = plan["samples_3x2x2x64x64"]
    assert p["fwd"] == (2, 2) and p["fwd_total"] == 24 and p["fwd_total"] % 8 == 0 and p["bwd_total"] % 8 == 0
    # both remap settings, both load widths, both parities each way
    assert {plan[n]["fwd_total"] % 8 == 0 for n in plan} == {True, False} and {plan[n]["bwd_total"] % 8 == 0 for n in plan} == {True, False}
    assert {plan[n]["odd"] for n in plan} >= {(0, 0), (0, 1), (1, 0), (1, 1)}
    # per-sample factors: powers of two, all different
    c = X.bwd_coef(3)
    assert c[0].tolist() == [0.5, 0.25] and c[1].tolist() == [2.0, 1.0] and len(set(c.flatten().tolist())) == 6


def test_pool_and_tmax_cases_reach_their_paths():
    big, tiny = X.pool_cases()
    quads = big["planes"] * X.cdiv(big["H"], 2) * X.cdiv(big["W"], 2)
    assert quads == 532512 > 2048 * 256 and big["H"] % 2 == 1 and big["W"] % 2 == 1 and big["planes"] * big["H"] * big["W"] * 4 < 8.5e6
    assert tiny["planes"] * 4 * 3 <= 256 and tiny["H"] % 2 == 1 and tiny["W"] % 2 == 1
    assert X.TMAX_N == (1, 3, 5, 1023, 3 * 8192 + 5)
    assert [X.tmax_plan(n, 0)["nblk"] for n in X.TMAX_N] == [1, 1, 1, 1, 4]
    for head in range(4):
        p = X.tmax_plan(X.TMAX_N[-1], head)
        assert p["h"] == head and 0 <= X.TMAX_N[-1] - p["t0"] <= 3 and p["t0"] == head + 4 * p["n4"]
        slot = X.tmax_slot_of(X.TMAX_N[-1], head)
        assert sorted(slot.unique().tolist()) == list(range(16))           # 4 workgroups x 4 waves, the other 48 slots stay -inf
        _, at = X.tmax_data(X.TMAX_N[-1], "last_wg", 0)
        assert int(slot[at]) // 4 == 3 and int(slot[0]) == 0 and int(slot[-1]) == 0
    assert X.tmax_plan(1, 3) == dict(h=1, n4=0, nblk=1, t0=1) and X.tmax_plan(5, 2)["n4"] == 0 and X.tmax_plan(5, 1)["n4"] == 1


def test_finalize_cases_cover_the_listed_settings():
    cs = X.finalize_cases()
    assert {c["B"] for c in cs} == {1, 3, 300} and {c["nscale"] for c in cs} == {1, 3, 5} and {c["slots"] for c in cs} == {1, 64}
    assert {c["gout"] is None for c in cs} == {True, False}
    assert any(c["a"][2] == 0 and c["a"][0] and not c["a"][1] for c in cs) and any(c["a"][2] == 0 and c["a"][1] and not c["a"][0] for c in cs)
    for c in cs:
        st = X.finalize_statement(c, X.finalize_fixture(c))   # asserts the two clamped means
        if st["coef"] is not None:
            assert int(st["clamped"].sum()) == 2 and st["k_coef"] == (2 * X.POW_ULP + 2) * c["nscale"] + 7


# ------------------------------------------------------------------------------------------------ 3. reference run
@pytest.mark.parametrize("case", X.stack_cases(), ids=_ids(X.stack_cases()))
def test_forward_cases_on_the_reference(case):
    X.run_forward_case(X.TorchEntry(), case, CPU)


@pytest.mark.parametrize("case", [c for c in X.stack_cases() if c["bwd"]], ids=_ids([c for c in X.stack_cases() if c["bwd"]]))
def test_backward_cases_on_the_reference(case):
    X.run_backward_case(X.TorchEntry(), case, CPU)


@pytest.mark.parametrize("case", X.chain_cases(), ids=_ids(X.chain_cases()))
def test_chain_cases_on_the_reference(case):
    X.run_chain_case(X.TorchEntry(), case, CPU)


def test_pool_tmax_and_finalize_cases_on_the_reference():
    ep = X.TorchEntry()
    for c in X.pool_cases():
        X.run_pool_case(ep, c, CPU)
    for n in X.TMAX_N:
        X.run_tmax_case(ep, n, CPU)
    for c in X.finalize_cases():
        X.run_finalize_case(ep, c, CPU)


# ------------------------------------------------------------------------------------------------ 4. the statement against the oracle
@pytest.mark.parametrize("name", ["edge_2x2x5x43x43", "one_pixel_1x3x1x11x11", "across_2x1x7x52x75", "grids_1x2x3x65x33"])
def test_statement_agrees_with_the_oracle(name):
    case = _case(name)
    fx, st = X.stack_fixture(case), X.case_statement(case)
    B = case["B"]
    ssim, cs = loss_ref.ssim_25d(fx["P"].float(), fx["T"].float())
    f = st["fields"][0]
    for got, ref in ((f["ssim"].v.reshape(B, -1).mean(1), ssim), (f["cs"].v.reshape(B, -1).mean(1), cs)):
        assert float((got - ref.double()).abs().max()) <= 1e-3 * float(ref.abs().max())
    # the gradient fields: float64 autograd of the oracle's formula on the same means
    for last in (0, 1):
        m = [t.clone().requires_grad_(True) for t in st["means"]]
        mx, my, mxx, myy, mxy = m
        sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
        cs64 = (2 * sxy + st["c2"]) / (sx + sy + st["c2"])
        ssim64 = ((2 * mx * my + st["c1"]) / (mx * mx + my * my + st["c1"])) * cs64
        g = torch.autograd.grad((ssim64 if last else cs64).sum(), [mx, mxx, mxy])
        for got, fname in zip(g, X.FIELDS):
            r = st["fields"][last][fname]
            assert float((got - r.v).abs().max()) <= 1e-12 * float(r.A.max()), (fname, last)


def test_entry_points_chain_into_the_oracle_loss():
    """the seven plain-PyTorch entry points, driven as viscy_amd/losses.py drives the library's, give the oracle's loss and gradient
    by the criteria of test_mixed_loss_vs_reference_golden, one-pass and two-pass"""
    pred, target, lr, gr = _old_inputs()
    for fused in (True, False):
        see = _old_criteria(X.TorchEntry(), pred, target, lr, gr, fused)
        assert not see, see


# ------------------------------------------------------------------------------------------------ 5. seeded defects
_OLD: dict = {}


def _old_inputs():
    if not _OLD:
        shape = (2, 2, 5, 192, 192)
        gen = torch.Generator().manual_seed(11)
        target = torch.rand(shape, generator=gen)
        pred = target + 0.1 * torch.randn(shape, generator=gen)
        pr = pred.clone().requires_grad_(True)
        lr = loss_ref.mixed_loss(pr, target, 0.5, 0.0, 0.5)
        lr.backward()
        _OLD.update(v=(pred, target, lr.item(), pr.grad))
    return _OLD["v"]


def _old_criteria(ep, pred, target, lr, gr, fused=True) -> list:
    """the assertions of test_mixed_loss_vs_reference_golden against the oracle run here; the list of those that fail"""
    l, g = X.mixed_loss_via(ep, pred, target, 0.5, 0.0, 0.5, fused)
    d = (g - gr).abs() / gr.abs().max()
    cos = torch.nn.functional.cosine_similarity(g.flatten().double(), gr.flatten().double(), dim=0).item()
    fails = [("loss", abs(l.item() - lr) <= 1e-3 * abs(lr)), ("grad_max", d.max().item() <= 1e-2),
             ("grad_tail", (d > 5e-3).float().mean().item() <= 1e-3), ("cosine", cos > 0.99999)]
    return [n for n, ok in fails if not ok]


def _exact_runner_fails(defect: str) -> str:
    """the first exact runner that fails on the defect, with the case it fails at"""
    ep = X.TorchEntry(defect)
    for c in X.stack_cases():
        for run in (X.run_forward_case,) + ((X.run_backward_case,) if c["bwd"] else ()):
            try:
                run(ep, c, CPU)
            except AssertionError as e:
                return f"{run.__name__} {c['name']}: {str(e)[:200]}"
    return ""


# defect -> (what the exact runners say, which of the old criteria fail at 192 x 192)
OLD_TESTS_SEE = {
    "l1_column_twice": ("L1 sum over the slots", []),
    "last_rows_unpooled": (" Po:", []),
    "coef_by_bc": ("ssim_scale_bwd_in", ["grad_max", "grad_tail", "cosine"]),   # seen at B = 2; at B = 1 there is nothing to mix up
    "coef_slots_swapped": ("ssim_scale_bwd_in", ["grad_max", "grad_tail", "cosine"]),
    "slot_left_out": ("sum_ssim", []),
    "dpnext_at_leftover": ("ssim_scale_bwd_in", []),
}


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_seeded_defect_fails_the_exact_runner_and_what_the_old_criteria_see(defect):
    msg = _exact_runner_fails(defect)
    assert msg and OLD_TESTS_SEE[defect][0] in msg, msg
    pred, target, lr, gr = _old_inputs()
    assert _old_criteria(X.TorchEntry(defect), pred, target, lr, gr) == OLD_TESTS_SEE[defect][1]


def test_defect_table_is_complete():
    assert set(OLD_TESTS_SEE) == set(X.DEFECTS) and sum(bool(v[1]) for v in OLD_TESTS_SEE.values()) == 2
