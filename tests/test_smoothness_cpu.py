"""CPU: the host half of viscy_amd.smoothness and the fixtures the GPU tests (tests/test_gpu_smoothness.py) stand on.

* the numpy restatements of tests/ref_smoothness.py reproduce the golden: the standardise restatement is array_equal to sklearn's
  fit_transform; the pair restatement, fed sklearn's mean_ / scale_, is within 4 (d + 8) 2^-53 of scipy's cdist (absolute for
  cosine, relative for Euclidean: both sides sum d exactly representable products in float64);
* the private RandomState(42) stream reproduces the reference's random distribution (cases C: a second batch, D: redraws);
* find_peaks_height equals scipy's find_peaks(height=) as recorded in the golden (hand-made signals, random plateaus, the curves);
* the golden KDE curves meet the conditions that make "equal peaks" a fair demand of the device: with B = 2 (n + 4096) 2^-53 the
  winner beats its neighbours and every other candidate by more than 2 B relative, and no value is within 2 B of 0.1 max;
* the vectorised pair builders equal plain Python loops."""

import functools

import numpy as np
import pytest

from tests import ref_smoothness as RS
from tests.conftest import load_golden
from viscy_amd import smoothness as S


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("smoothness.pt")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x, obs, metric, offsets, z from sklearn's mean_ / scale_, pi, pj)"""
    x, obs, metric, offsets = RS.build(name)
    g = golden()["cases"][name]
    z = RS.standardize(x, g["mean_"].numpy(), g["scale_"].numpy())
    pi, pj, _, _ = S.adjacent_pairs(obs["fov_name"], obs["track_id"], offsets)
    return x, obs, metric, offsets, z, pi, pj


def close(name, got, want, d, metric):
    err = np.abs(got - want)
    bound = RS.pair_bound(d) * (np.abs(want) if metric == "euclidean" else 1.0)
    assert (err <= bound).all(), (name, float(err.max()), float(np.max(bound)))


RUNNING = [n for n in RS.CASES if n != "F"]


@pytest.mark.parametrize("name", [n for n in RS.CASES if len(RS.build(n)[0]) <= 64])
def test_standardize_restatement_is_sklearn(name):
    z = case(name)[4]
    want = golden()["cases"][name]["z"].numpy()
    assert z.dtype == want.dtype == np.float32 and np.array_equal(z, want)
    if name == "H":
        assert (z[:, RS.CASES["H"]["constant_column"]] == 0.0).all() and golden()["cases"]["H"]["scale_"][2] == 1.0


@pytest.mark.parametrize("name", RUNNING)
def test_pair_restatement_reproduces_the_reference(name):
    x, obs, metric, offsets, z, pi, pj = case(name)
    g = golden()["cases"][name]
    ri, rj = S.random_pairs(len(x), len(pi))
    adj, rnd = RS.pair_dist(z, pi, pj, metric), RS.pair_dist(z, ri, rj, metric)
    if name == "C":
        assert len(pi) == g["n_pairs"] > 10000      # a second random batch is drawn
        for got, key in ((adj, "adjacent"), (rnd, "random")):
            close(name, got[::16], g[key + "_s16"].numpy(), x.shape[1], metric)
            close(name, got[9936:10064], g[key + "_mid"].numpy(), x.shape[1], metric)
    else:
        close(name, adj, g["adjacent"].numpy(), x.shape[1], metric)
        close(name, rnd, g["random"].numpy(), x.shape[1], metric)


def test_random_stream_is_the_references():
    for n, p in ((12000, 11582), (3, 3), (40, 62)):
        i, j = S.random_pairs(n, p)
        ri, rj, _ = RS.random_pairs(n, p)
        assert np.array_equal(i, ri) and np.array_equal(j, rj) and (i != j).all() and i.dtype == np.int64
    # D: the reference's own run needed redraws (the generator counted its np.random.randint calls), as many passes as the
    # restated stream takes; what pins the stream itself is the match of the random distances in the test above
    for name, n, p in (("D", 3, 3), ("C", 12000, 11582), ("B", 40, 62)):
        assert golden()["cases"][name]["redraws"] == RS.random_pairs(n, p)[2]
    assert golden()["cases"]["D"]["redraws"] > 0
    state = np.random.get_state()
    S.random_pairs(100, 50)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


@pytest.mark.parametrize("y,height,want", RS.HAND_MADE_PEAKS)
def test_find_peaks_known_answers(y, height, want):
    assert S.find_peaks_height(np.array(y, dtype=np.float64), height).tolist() == want


def test_find_peaks_equals_scipys_recorded_peaks():
    """scipy.signal.find_peaks(y, height=0.1 max y) as the generator recorded it: the hand-made signals, 20 random signals of many
    plateaus, and the two 1000-point curves of case A"""
    rec = golden()["find_peaks"]
    signals = RS.peak_signals()
    assert len(signals) == len(rec["signals"]) == len(RS.HAND_MADE_PEAKS) + 20
    for y, want in zip(signals, rec["signals"]):
        assert S.find_peaks_height(y, 0.1 * y.max()).tolist() == want, y
    assert sum(len(w) for w in rec["signals"]) > 100      # the random signals do have peaks
    for key in ("adjacent", "random"):
        y = golden()["curves"][key].numpy()
        assert S.find_peaks_height(y, 0.1 * y.max()).tolist() == rec["curves"][key] != []


@pytest.mark.parametrize("key", ["adjacent", "random"])
def test_golden_curves_decide_their_peak(key):
    g = golden()
    data, curve = g["cases"]["A"][key].numpy(), g["curves"][key].numpy()
    grid = np.linspace(data.min(), data.max(), RS.GRID)
    peaks = S.find_peaks_height(curve, 0.1 * curve.max())
    assert len(peaks) >= 1
    win = peaks[np.argmax(curve[peaks])]
    assert grid[win] == g["cases"]["A"]["stats"][key + "_frame_peak"]
    B2 = 2.0 * RS.kde_bound(len(data))
    top = curve[win]
    assert curve[win - 1] < top * (1 - B2) and curve[win + 1] < top * (1 - B2)
    for p in S.find_peaks_height(curve, 0.0):    # every local maximum is a candidate once values move by B
        assert p == win or curve[p] < top * (1 - B2)
    thr = 0.1 * curve.max()
    assert (np.abs(curve - thr) > B2 * thr).all()
    # the restated normalisation of the float64 sums is scipy's curve
    want = RS.kde_curve(data, RS.kde_sums(data, grid, RS.kde_a(data)).astype(np.float64))
    assert np.allclose(want, curve, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", list(RS.CASES))
def test_adjacent_pairs_equal_the_double_loop(name):
    x, obs, metric, offsets = RS.build(name)
    pi, pj, piecewise, splits = S.adjacent_pairs(obs["fov_name"], obs["track_id"], offsets)
    wi, wj, pieces = RS.adjacent_pairs_loop(obs["fov_name"], obs["track_id"], offsets)
    assert np.array_equal(pi, wi) and np.array_equal(pj, wj)
    got = [p.tolist() for p in np.split(piecewise, splits)] if len(piecewise) else []
    assert got == pieces
    g = golden()["cases"][name]
    if g["error"] is None:
        assert [len(p) for p in pieces] == g["piecewise_lengths"]
    else:
        assert len(pi) == 0 and g["error"][0] == "ValueError"
    # a DataFrame's columns give the same lists
    ad, _, _ = RS.adata(name, frame=True)
    fi, fj, _, _ = S.adjacent_pairs(ad.obs["fov_name"], ad.obs["track_id"], offsets)
    assert np.array_equal(fi, pi) and np.array_equal(fj, pj)


def test_adjacent_pairs_refuse_an_offset_below_one():
    with pytest.raises(ValueError, match="time_offsets must be positive"):
        S.adjacent_pairs(np.array(["a", "a"]), np.array([0, 0]), [0])


def test_track_pairs_equal_the_plain_loop():
    ds = RS.msd_dataset()
    rows, starts, lengths = S.track_pairs(ds["fov_name"], ds["track_id"], ds["t"])
    seen, taus = [], {}
    for f, k in zip(ds["fov_name"], ds["track_id"]):
        if (f, k) not in seen:
            seen.append((f, k))
    assert len(seen) == len(starts) and 1 in lengths.tolist()
    cache = {}
    for (f, k), s, T in zip(seen, starts, lengths):
        mine = np.flatnonzero((ds["fov_name"] == f) & (ds["track_id"] == k))
        mine = mine[np.argsort(ds["t"][mine], kind="stable")]
        assert np.array_equal(rows[s:s + T], mine)
        if T > 1:
            i, j = S._offset_major(int(T), cache)
            want = [(a, a + off) for off in range(1, T) for a in range(T - off)]
            assert list(zip(i.tolist(), j.tolist())) == want
            for a, b in want:
                taus.setdefault(int(ds["t"][mine[b]] - ds["t"][mine[a]]), []).append(1)
    for metric in ("cosine", "euclidean"):
        rec = golden()["msd"][metric]
        assert [tau for tau, _ in rec] == list(taus) and [len(v) for _, v in rec] == [len(v) for v in taus.values()]
    assert any(np.diff(ds["t"][rows[s:s + T]]).max() > 1 for s, T in zip(starts, lengths) if T > 1)   # non-unit steps


def test_host_side_exceptions_and_histogram():
    err = golden()["errors"]
    types = {"ValueError": ValueError, "LinAlgError": np.linalg.LinAlgError}
    for key, data in RS.DEGENERATE.items():
        with pytest.raises(types[err[key][0]]) as e:
            S.find_distribution_peak(data)
        assert type(e.value).__name__ == err[key][0] and str(e.value) == err[key][1], key
    with pytest.raises(ValueError) as e:
        S.find_distribution_peak(np.arange(5.0), method="mode")
    assert str(e.value) == err["unknown_method"][1]
    g = golden()
    for key in ("adjacent", "random"):
        assert S.find_distribution_peak(g["cases"]["A"][key].numpy(), method="histogram") == g["curves"][key + "_hist_peak"]


def test_pair_indices_are_checked_before_they_are_narrowed():
    import torch

    x = torch.zeros(3, 2)
    for pi, pj in (([0, 3], [1, 1]), ([0, 1], [-1, 1]), ([2 ** 31], [0])):
        with pytest.raises(ValueError, match="pair indices must lie in"):
            S._pair_dist(x, np.array(pi), np.array(pj), "cosine", 0.0)
