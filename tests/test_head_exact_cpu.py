"""CPU: the exact-arithmetic fixtures of tests/ref_exact_head.py without a GPU.

1. every case of the tables runs through the plain-PyTorch statements of tests/ref_ops.py (tests/ref_ops_narrow.py for the narrow
   voxel shuffle) and is bit-equal to the float64 statement: this checks the statements against a second formulation (the
   convolution tap by tap from the layouts of headconv.hip against F.conv3d and torch.nn.grad) and the exactness budgets;
2. the tables reach what they claim to reach, from the dispatch arithmetic of the entry points: tiles_per_wg and the grid cap
   512 of the convolution, rows_per_wg and the three tiers of the head shuffle, the element-count threshold of the voxel shuffle;
3. sensitivity: the reference namespace wrapped in mutants, each of which makes ONE indexing error, fails its runner;
4. what the tolerance tests of tests/test_gpu_ops.py make of the same mutants on that file's own operands and shapes, recorded
   per mutant in OLD_TESTS_SEE and asserted, so the stated gap stays true: they see six of the seven; the one they cannot see
   lives on a path (a second tile per workgroup) that none of their shapes executes."""

import re
import types

import pytest
import torch

from tests import ref_exact_head as X
from tests import ref_ops_narrow as R

CPU = torch.device("cpu")
BF16, F32 = X.BF16, X.F32


def _with(cases, inner):
    return [pytest.param(c, i, id=f"{c['name']}-{i}") for c in cases for i in inner(c)]


def _case(cases, name):
    return next(c for c in cases if c["name"] == name)


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()


# ------------------------------------------------------------------------------------------------ 1. reference run
@pytest.mark.parametrize("case,part", _with(X.conv_cases(), lambda c: X.CONV_PARTS))
def test_conv_cases_on_the_reference(case, part):
    X.run_conv_case(R, case, part, CPU)


@pytest.mark.parametrize("case,direction", _with(X.shuffle_cases(), lambda c: ("fwd", "bwd")))
def test_shuffle_cases_on_the_reference(case, direction):
    X.run_shuffle_case(R, case, direction, CPU)


@pytest.mark.parametrize("case,direction", _with(X.voxel_cases(), lambda c: c["dirs"]))
def test_voxel_cases_on_the_reference(case, direction):
    X.run_voxel_case(R, case, direction, CPU)


# ------------------------------------------------------------------------------------------------ 2. the tables
class _Lib:
    """a library that only knows its flags (head_rows as shipped: 63)"""

    def __init__(self):
        self.flags = {b"head_rows": 63}

    def vsx_get_flag(self, name):
        return self.flags[name]

    def vsx_set_flag(self, name, value):
        self.flags[name] = value
        return 0


def test_convolution_cases_reach_the_paths_they_are_listed_for():
    cases = X.conv_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    plan = {c["name"]: X.conv_plan(c["B"], c["H2"], c["W2"]) for c in cases}
    for c in cases:   # what the entry points accept, the sample size of the statistics budget, the quoted arithmetic
        p = plan[c["name"]]
        assert c["H2"] % 16 == 0 and c["W2"] % 16 == 0 and c["H2"] * c["W2"] <= 64 * 64
        assert f"cdiv({p['ntiles']}, 512) = {p['tiles_per_wg']}" in c["leg"] and f"min(ntiles, 512) = {p['wgrad_grid']}" in c["leg"]
    # one tile column: both borders in the same tile, two tile rows
    one = _case(cases, "one_tile_column_2x16x16")
    assert (one["H2"], one["W2"]) == (16, 16) and one["B"] >= 2
    assert plan[one["name"]]["tiles_x"] == 1 and plan[one["name"]]["tiles_y"] == 2
    # interior tiles: one with all eight neighbours
    assert any(p["tiles_x"] >= 3 and p["tiles_y"] >= 4 for p in plan.values())
    # persistent ranges
    p = plan["persistent_37x32x112"]
    assert p["ntiles"] == 1036 > 1024 and p["tiles_per_wg"] == -(-p["ntiles"] // 512) >= 3
    assert p["per_sample"] % p["tiles_per_wg"] != 0 and p["tiles_x"] % p["tiles_per_wg"] != 0   # ranges cross samples and tile rows
    assert p["ntiles"] % p["tiles_per_wg"] != 0 and p["last"] == 1 and p["wgs"] == 346          # a short last range
    assert p["ntiles"] > 512 and p["wgrad_grid"] == 512 and (p["wgrad_min"], p["wgrad_max"]) == (2, 3)   # two and three tiles
    assert p["ntiles"] % 512 != 0
    # every other case leaves these paths alone, as the existing tolerance tests do
    assert all(q["tiles_per_wg"] == 1 and q["wgrad_max"] == 1 for n, q in plan.items() if n != "persistent_37x32x112")
    # the four forward settings; the flag comes back
    lib = _Lib()
    flags = X.Flags(lib)
    var = X.conv_fwd_variants(flags)
    assert sorted((s["head_rows"] & 32, det) for s, det in var) == [(0, False), (0, True), (32, False), (32, True)]
    assert all(s["head_rows"] | 32 == 63 for s, _ in var)
    with flags.scoped(var[-1][0]):
        assert lib.flags[b"head_rows"] == 31
    assert lib.flags[b"head_rows"] == 63
    assert X.conv_fwd_variants(X.Flags()) == [({}, False)]
    # zero handling: asserted when the fixture is made; shown here on the smallest case
    fx = X.conv_fixture(one)
    for w in (fx["w_par"], fx["w_par_g"]):
        assert bool((X.prepared(w) != 0).any(0).all()) and X.prepared(w).shape == (32, 216)
    assert float(fx["hin"].abs().max()) == 1 and float(fx["w_par"].abs().max()) == 1 and float(fx["dU"].abs().max()) == 2


def test_convolution_budgets_hold_on_the_statements():
    """max |U| <= 256 and sum c^2 < 2^24 per (sample, channel) are asserted where the statement is made; the margins"""
    for c in X.conv_cases()[:2]:
        st = X.conv_statement(c, "fwd")
        assert st["umax"] <= 27 * 8 + 8 and st["sqmax"] < X.LIMIT / 8
        assert 4 * c["B"] * c["H2"] * c["W2"] * 5 + 24 < X.LIMIT
    big = X.conv_cases()[2]
    assert 4 * big["B"] * big["H2"] * big["W2"] * 5 + 24 < X.LIMIT


def test_shuffle_cases_reach_every_tier():
    cases = X.shuffle_cases()
    plan = lambda c, dt, pool, **kw: X.shuffle_plan(c["B"], c["h"], c["w"], c["c3"], c["D"], dt, pool, **kw)
    tiled = _case(cases, "tiled_2x9x11")
    assert tiled["B"] >= 2 and all(tiled[k] % 8 and tiled[k] % 4 for k in ("h", "w"))
    for dt in X.BOTH:
        for pool in (True, False):
            p = plan(tiled, dt, pool)
            assert p["tier"] == "tiled" and min(p["tiles"]) >= 2
    strips = [c for c in cases if c["sweep"]]
    for c in strips:
        assert c["c3"] * c["D"] == 56 and c["w"] % 64 == 0 and BF16 in c["dts"] and True in c["pools"]
        for bwd in (False, True):
            assert plan(c, BF16, True, bwd=bwd)["tier"] == "strip"
            assert plan(c, BF16, True, head_rows=63 & ~24, bwd=bwd)["tier"] == "tiled"    # the sweep's other setting
            assert plan(c, BF16, False, bwd=bwd)["tier"] == "tiled" and plan(c, F32, True, bwd=bwd)["tier"] == "tiled"
        var = X.shuffle_variants(c, BF16, True, X.Flags(_Lib()))
        assert [v["head_rows"] & 24 for v in var] == [24, 0]
        assert X.shuffle_variants(c, F32, True, X.Flags(_Lib())) == [{}] and X.shuffle_variants(c, BF16, False, X.Flags(_Lib())) == [{}]
    a = _case(cases, "strips_2x20x192")
    p = plan(a, BF16, True)
    assert a["w"] == 192 and a["h"] == 20 and p["rows_per_wg"] == 8 and p["ranges"] == 3   # x0 = 0, 64, 128; y0 = 0, 8, 16
    b = _case(cases, "strips_rows9_72x64x64")
    p = plan(b, BF16, True)
    assert b["h"] * p["strips"] >= 4608 and p["rows_per_wg"] == b["h"] * p["strips"] // 512 == 9 and b["h"] % p["rows_per_wg"] != 0
    assert "= 9" in b["leg"]
    t = _case(cases, "thread_per_element_2x5x7_d9")
    assert t["c3"] * t["D"] > 64 and (t["c3"] * t["D"]) % 8 == 0
    assert all(plan(t, dt, pool, bwd=bwd)["tier"] == "thread" for dt in X.BOTH for pool in (True, False) for bwd in (True, False))
    assert set(t["dts"]) == set(X.BOTH) and set(t["pools"]) == {True, False}


def test_voxel_cases_reach_the_stride_loop_and_the_narrow_kernel():
    cases = X.voxel_cases()
    plain = [c for c in cases if not c["narrow"] and set(c["dirs"]) == {"fwd", "bwd"}]
    assert {c["s"] for c in plain} == {2, 4}
    for c in plain:
        assert c["B"] >= 2 and c["h"] % 2 == 1 and c["w"] % 2 == 1 and set(c["pools"]) == {True, False} and set(c["dts"]) == set(X.BOTH)
        assert c["cd"] % 8 == 0   # what vsx_voxel_shuffle_bwd asks of bf16
    outs = lambda c: c["B"] * c["cd"] * c["h"] * c["w"]
    big = [c for c in cases if "fwd" in c["dirs"] and outs(c) > 65536 * 256]
    assert big and all(X.voxel_passes(outs(c)) == 2 for c in big)
    assert all(X.voxel_passes(outs(c)) == 1 for c in plain)
    narrow = [c for c in cases if c["narrow"]]
    assert narrow and all(c["cd"] % 8 != 0 and c["dirs"] == ("bwd",) for c in narrow) and any(c["cd"] < 8 for c in narrow)
    assert any(X.voxel_passes(outs(c)) == 2 for c in narrow)   # one thread per element
    # the vector kernel's own stride loop is out of reach of a quick test: more than 65536 * 256 vectors of 8
    assert all(outs(c) // 8 <= 65536 * 256 for c in cases if "bwd" in c["dirs"] and not c["narrow"])


def test_outputs_start_as_nan_inside_the_runner():
    real = torch.empty
    with pytest.raises(RuntimeError, match="inside"):
        with X.nan_outputs():
            t, i = torch.empty(4, 3), torch.empty(2, dtype=torch.long)
            raise RuntimeError("inside")
    assert bool(torch.isnan(t).all()) and i.dtype == torch.long
    assert torch.empty is real   # put back, also after an exception


# ------------------------------------------------------------------------------------------------ 3. sensitivity
def _mutant(**over):
    ns = types.SimpleNamespace(**{k: getattr(R, k) for k in dir(R) if not k.startswith("__")})
    ns.__dict__.update(over)
    return ns


def _store(U5, dtype, ssum, ssq):
    """round, form the statistics of what is stored, hand back [M, zo * cmid]"""
    B, cmid = U5.shape[0], U5.shape[-1]
    U = U5.to(dtype)
    s = U.float().view(B, -1, cmid)
    ssum += s.sum(1)
    ssq += (s * s).sum(1)
    return U.view(-1, U5.shape[3] * cmid)


def _fwd5(hin, Wc, bias, B, H2, W2, c3, cmid, zo):
    z = torch.zeros(B, cmid)
    return R.head_conv_fwd(hin, Wc, bias, z, z.clone(), B, H2, W2, c3, cmid, zo).float().view(B, H2, W2, zo, cmid)


def reads_the_wrong_plane_for_one_tap():
    """output plane 2 reads input plane 4 where the tap (dy 1, dx 1, dz 1) wants plane 3: one tap's dz offset, one plane"""
    def head_conv_fwd(hin, Wc, bias, ssum, ssq, B, H2, W2, c3, cmid, zo):
        U = _fwd5(hin, Wc, bias, B, H2, W2, c3, cmid, zo)
        x, W = hin.float().view(B, H2, W2, zo + 2, c3), Wc.float().view(cmid, 3, 3, 3, c3)
        U[:, :, :, 2, :] += (x[:, :, :, 4, :] - x[:, :, :, 3, :]) @ W[:, 1, 1, 1, :].t()
        return _store(U, hin.dtype, ssum, ssq)
    return _mutant(head_conv_fwd=head_conv_fwd)


def zeroes_the_right_halo_one_column_early():
    """the last tile column stages x < W2 - 1 instead of x < W2: its column W2 - 1 is zero for every tap"""
    def head_conv_fwd(hin, Wc, bias, ssum, ssq, B, H2, W2, c3, cmid, zo):
        x = hin.clone().view(B, H2, W2, -1)
        x[:, :, W2 - 1] = 0
        return R.head_conv_fwd(x.view(hin.shape), Wc, bias, ssum, ssq, B, H2, W2, c3, cmid, zo)
    return _mutant(head_conv_fwd=head_conv_fwd)


def credits_one_tile_to_the_next_sample():
    """the InstanceNorm partials of the last tile (8 x 16 pixels) of sample 0 are added to sample 1"""
    def head_conv_fwd(hin, Wc, bias, ssum, ssq, B, H2, W2, c3, cmid, zo):
        U = R.head_conv_fwd(hin, Wc, bias, ssum, ssq, B, H2, W2, c3, cmid, zo)
        if B > 1:
            t = U.float().view(B, H2, W2, zo, cmid)[0, H2 - 8:, W2 - 16:].reshape(-1, cmid)
            for acc, v in ((ssum, t.sum(0)), (ssq, (t * t).sum(0))):
                acc[0] -= v
                acc[1] += v
        return U
    return _mutant(head_conv_fwd=head_conv_fwd)


def wgrad_stops_at_the_grid():
    """the weight gradient's workgroups take one tile each: tiles t >= 512 are never visited"""
    def head_conv_wgrad(hin, dU, dW, db, B, H2, W2, c3, cmid, zo):
        b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), indexing="ij")
        t = (b * (H2 // 8) + y // 8) * (W2 // 16) + x // 16
        g = dU * (t.reshape(-1, 1) < 512).to(dU.dtype)
        return R.head_conv_wgrad(hin, g, dW, db, B, H2, W2, c3, cmid, zo)
    return _mutant(head_conv_wgrad=head_conv_wgrad)


def dgrad_plane_6_uses_the_wrong_dz():
    """input plane z' = 6 gets its one contribution (z = 4) through the weights of dz = 1 instead of dz = 2"""
    def head_conv_dgrad(dU, Wp, B, H2, W2, c3, cmid, zo):
        good = R.head_conv_dgrad(dU, Wp, B, H2, W2, c3, cmid, zo).view(-1, zo + 2, c3).clone()
        W = Wp.clone().view(cmid, 3, 3, 3, c3)
        W[:, :, :, 2, :] = W[:, :, :, 1, :]
        good[:, zo + 1] = R.head_conv_dgrad(dU, W.view(Wp.shape), B, H2, W2, c3, cmid, zo).view(-1, zo + 2, c3)[:, zo + 1]
        return good.view(-1, (zo + 2) * c3)
    return _mutant(head_conv_dgrad=head_conv_dgrad)


def _shuffle_with(column=None, row=None):
    """output column 2 * (column + 1) / row 2 * (row + 1) of the pooled forward without decoder column / row ``column`` / ``row``"""
    def head_shuffle_fwd(dec, B, h, w, C3, D, pool):
        out = R.head_shuffle_fwd(dec, B, h, w, C3, D, pool).view(B, 2 * h, 2 * w, -1).clone()
        d = dec.clone().view(B, h, w, -1)
        if pool and column is not None and w > column + 1:
            d[:, :, column] = 0
            out[:, :, 2 * column + 2] = R.head_shuffle_fwd(d.view(dec.shape), B, h, w, C3, D, pool).view(out.shape)[:, :, 2 * column + 2]
        if pool and row is not None and h > row + 1:
            d[:, row] = 0
            out[:, 2 * row + 2] = R.head_shuffle_fwd(d.view(dec.shape), B, h, w, C3, D, pool).view(out.shape)[:, 2 * row + 2]
        return out.view(B * 4 * h * w, -1)
    return _mutant(head_shuffle_fwd=head_shuffle_fwd)


def zeroes_the_left_halo_of_the_second_strip():
    """the strip at x0 = 64 gets zeros for decoder column 63: output column 128 pools without its left neighbours"""
    return _shuffle_with(column=63)


def drops_the_carried_row_of_the_second_range():
    """the row range at y0 = 8 starts with empty carries: output row 16 pools without decoder row 7"""
    return _shuffle_with(row=7)


MUTANTS = {
    "wrong_plane_for_one_tap": (reads_the_wrong_plane_for_one_tap, "conv", "interior_2x32x48", "fwd", r"forward.* U "),
    "right_halo_one_column_early": (zeroes_the_right_halo_one_column_early, "conv", "one_tile_column_2x16x16", "fwd", r"forward.* U "),
    "tile_statistics_on_next_sample": (credits_one_tile_to_the_next_sample, "conv", "interior_2x32x48", "fwd", r"ssum"),
    "wgrad_skips_tiles_from_512": (wgrad_stops_at_the_grid, "conv", "persistent_37x32x112", "wgrad", r" dW "),
    "dgrad_plane_6_wrong_dz": (dgrad_plane_6_uses_the_wrong_dz, "conv", "one_tile_column_2x16x16", "dgrad", r" dhin "),
    "left_halo_zeroed_at_x0_64": (zeroes_the_left_halo_of_the_second_strip, "shuffle", "strips_2x20x192", "fwd", r"head_shuffle_fwd"),
    "carried_row_dropped": (drops_the_carried_row_of_the_second_range, "shuffle", "strips_2x20x192", "fwd", r"head_shuffle_fwd"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_exact_runner_catches_the_mutant(name):
    make, family, case_name, part, match = MUTANTS[name]
    if family == "conv":
        case = _case(X.conv_cases(), case_name)
        X.run_conv_case(R, case, part, CPU)
        with pytest.raises(AssertionError, match=match) as e:
            X.run_conv_case(make(), case, part, CPU)
    else:
        case = _case(X.shuffle_cases(), case_name)
        with pytest.raises(AssertionError, match=match) as e:
            X.run_shuffle_case(make(), case, part, CPU)
    assert "elements differ" in str(e.value) and "got" in str(e.value)   # the report names the first mismatching element


def test_a_mutant_beyond_the_grid_is_invisible_below_512_tiles():
    """the weight gradient that stops at its grid is the correct one on every shape with at most 512 tiles: only the large case
    can tell them apart"""
    for name in ("one_tile_column_2x16x16", "interior_2x32x48"):
        X.run_conv_case(wgrad_stops_at_the_grid(), _case(X.conv_cases(), name), "wgrad", CPU)


def test_mismatch_report_names_pixel_plane_and_channel():
    case = _case(X.conv_cases(), "one_tile_column_2x16x16")
    with pytest.raises(AssertionError) as e:
        X.run_conv_case(dgrad_plane_6_uses_the_wrong_dz(), case, "dgrad", CPU)
    text = str(e.value)
    assert "ch = plane * 8 + channel" in text and "columns 48 .. 55" in text   # plane 6 only
    assert re.search(r"\(b 0, z 0, y \d+, x \d+, ch (4[89]|5[0-5])\): got ", text)


# ------------------------------------------------------------------------------------------------ 4. the gap
def _failed(checks):
    bad = []
    for name, fn in checks:
        try:
            fn()
        except AssertionError:
            bad.append(name)
    return bad


def old_head_conv_test(H, B, gh, gw):
    """the comparisons of tests/test_gpu_ops.py::test_head_conv_direct_bf16 on its operands, with ``H`` in the place of the HIP ops
    and the CPU statements in the place of the z-batched GEMM path: the names of the comparisons that fail"""
    from tests.test_gpu_ops import close, rnd

    dt, c3, cmid, Zo = BF16, 8, 32, 5
    D7, Mh = Zo + 2, B * gh * gw
    hin, Wc, bias = rnd(Mh, D7 * c3, dt=dt, seed=1), rnd(cmid, c3, 3, 3, 3, seed=2, scale=0.1), rnd(cmid, seed=3)
    dU = rnd(Mh, Zo * cmid, dt=dt, seed=4)
    Wg, _ = H.prep_weight(Wc, cmid, c3, 27, dt, tapmode=1)
    st = torch.zeros(2, B, cmid)
    U = H.head_conv_fwd(hin, Wg, bias, st[0], st[1], B, gh, gw, c3, cmid, Zo)
    dWc, db, dWp = torch.zeros(cmid, 27 * c3), torch.zeros(cmid), torch.zeros(cmid, c3, 3, 3, 3)
    H.head_conv_wgrad(hin, dU, dWc, db, B, gh, gw, c3, cmid, Zo)
    H.unprep_grad(dWc, dWp, cmid, c3, 27, tapmode=1)
    dhin = H.head_conv_dgrad(dU, H.head_conv_dgrad_prep(Wg), B, gh, gw, c3, cmid, Zo)
    x5 = hin.float().view(B, gh, gw, D7, c3).permute(0, 4, 3, 1, 2).clone().requires_grad_(True)
    w, bb = Wc.to(dt).float().clone().requires_grad_(True), bias.clone().requires_grad_(True)
    with torch.enable_grad():
        y = torch.nn.functional.conv3d(x5, w, bb, padding=(0, 1, 1))
        y.backward(dU.float().view(B, gh, gw, Zo, cmid).permute(0, 4, 3, 1, 2))
    Uref = y.detach().permute(0, 3, 4, 2, 1).reshape(Mh, Zo * cmid)
    ur = Uref.to(dt).float().view(B, gh * gw * Zo, cmid)
    U2, st2 = torch.zeros(Mh, Zo * cmid, dtype=dt), torch.zeros(2, B, cmid)
    R.gemm_z("nt", hin, Wg, U2, Mh, cmid, 27 * c3, D7 * c3, 27 * c3, Zo * cmid, dtype=dt, a_mode=R.A_CONV3, gh=gh, gw=gw, cs=3 * c3, nz=Zo,
             a_coff=[z * c3 for z in range(Zo)], b_off=[0] * Zo, c_coff=[z * cmid for z in range(Zo)], epi=R.EPI_BIAS_STATS, bias=bias,
             red0=st2[0], red1=st2[1], hw=gh * gw)

    def one_ulp():
        assert (U.float() - U2.float()).abs().max().item() <= 2.0 ** -7 * U2.float().abs().max().item()

    return _failed([
        ("U", lambda: close(U, Uref, dt)), ("sum", lambda: close(st[0], ur.sum(1), dt)), ("sumsq", lambda: close(st[1], (ur * ur).sum(1), dt)),
        ("dW", lambda: close(dWp, w.grad, dt)), ("db", lambda: close(db, bb.grad, dt)),
        ("dhin", lambda: close(dhin, x5.grad.permute(0, 3, 4, 2, 1).reshape(Mh, D7 * c3), dt)),
        ("U against the GEMM path", one_ulp), ("statistics against the GEMM path", lambda: torch.testing.assert_close(st, st2, rtol=2e-3, atol=2e-2)),
    ])


def old_head_shuffle_test(H, geom):
    """the comparisons of tests/test_gpu_ops.py::test_head_shuffle (pooled, bf16) on its operands"""
    from tests.test_gpu_ops import close, rnd

    (B, h, w), C3, D, dt = geom, 8, 7, BF16
    dec, dh = rnd(B * h * w, 4 * C3 * D, dt=dt, seed=1), rnd(B * 4 * h * w, C3 * D, dt=dt, seed=2)
    return _failed([
        ("fwd", lambda: close(H.head_shuffle_fwd(dec, B, h, w, C3, D, True), R.head_shuffle_fwd(dec, B, h, w, C3, D, True), dt)),
        ("bwd", lambda: close(H.head_shuffle_bwd(dh, B, h, w, C3, D, True), R.head_shuffle_bwd(dh, B, h, w, C3, D, True), dt)),
    ])


# per mutant: the comparisons of the old tests that fail on it, on the largest shape of those tests that the mutant touches
# ((2, 32, 48) of test_head_conv_direct_bf16, (1, 20, 128) of test_head_shuffle); () = the old tests pass on the mutant
OLD_TESTS_SEE = {
    "wrong_plane_for_one_tap": ("U", "U against the GEMM path", "statistics against the GEMM path"),
    "right_halo_one_column_early": ("U", "U against the GEMM path", "statistics against the GEMM path"),
    "tile_statistics_on_next_sample": ("sum", "sumsq", "statistics against the GEMM path"),
    "wgrad_skips_tiles_from_512": (),
    "dgrad_plane_6_wrong_dz": ("dhin",),
    "left_halo_zeroed_at_x0_64": ("fwd",),
    "carried_row_dropped": ("fwd",),
}


def test_the_old_tests_pass_on_the_reference():
    assert old_head_conv_test(R, 2, 32, 48) == [] and old_head_conv_test(R, 1, 16, 16) == []
    assert old_head_shuffle_test(R, (1, 20, 128)) == []


@pytest.mark.parametrize("name", list(MUTANTS))
def test_what_the_tolerance_tests_make_of_the_mutant(name):
    """OLD_TESTS_SEE is a record, not a requirement.  What it shows: ``close()`` is a max-norm over elements (2e-2 of the tensor's
    largest value), and on random-normal operands a whole tap, a zeroed halo column or a dropped carried row moves single
    elements by far more than that, so six of the seven mutants are seen wherever the old shapes execute the faulty path; a tile
    is 1 / 12 of a sample of the (2, 32, 48) shape, so its statistics on the wrong sample are seen too.  The seventh is the gap
    itself: no old shape has a second tile per workgroup, so a weight gradient that stops at its grid passes every comparison.
    The same holds for every path the old shapes never run (tiles_per_wg > 1, head_rows bit 5 cleared, rows_per_wg > 8, the
    thread-per-element tier, the stride loops): the exact tests are needed for their shapes and settings first, and for their
    bit equality where an error is smaller than a tap (one product, one row of a reduction)."""
    make, family = MUTANTS[name][0], MUTANTS[name][1]
    got = old_head_conv_test(make(), 2, 32, 48) if family == "conv" else old_head_shuffle_test(make(), (1, 20, 128))
    print(name, "->", got)
    assert tuple(got) == OLD_TESTS_SEE[name]
