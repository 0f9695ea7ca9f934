"""bench.py host logic that needs no GPU: the N-rank launcher (`--gpus N` must either run N ranks or fail — VERDICT r3 item 2)
and the kernel-family naming shared by the live timing table, tools/roofline_table.py and tools/pmc_traffic.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_resolve_world_single_process():
    assert bench.resolve_world(1, {}, 0) == ("run", 1)
    assert bench.resolve_world(1, {}, 8) == ("run", 1)
    assert bench.resolve_world(8, {}, 8) == ("spawn", 8)
    assert bench.resolve_world(2, {}, 8) == ("spawn", 2)


def test_resolve_world_refuses_what_it_cannot_honour():
    with pytest.raises(SystemExit) as e:
        bench.resolve_world(2, {}, 1)  # one visible GPU: never an n_gpus = 1 line for a --gpus 2 request
    assert e.value.code not in (0, None)
    with pytest.raises(SystemExit):
        bench.resolve_world(8, {"WORLD_SIZE": "4"}, 8)  # launcher and flag disagree
    with pytest.raises(SystemExit):
        bench.resolve_world(4, {"WORLD_SIZE": "4"}, 2)  # more ranks than devices
    with pytest.raises(SystemExit):
        bench.resolve_world(0, {}, 8)


def test_resolve_world_under_the_driver_launcher():
    # the driver's N > 1 form: torch.distributed.run sets WORLD_SIZE, every rank gets the same --gpus N
    assert bench.resolve_world(8, {"WORLD_SIZE": "8"}, 8) == ("run", 8)
    assert bench.resolve_world(1, {"WORLD_SIZE": "1"}, 1) == ("run", 1)


def test_launch_command_is_the_documented_form():
    cmd = bench.launch_command(4, ["--gpus", "4", "--steps", "7", "--dry-launch", "--warmup", "2"], port=29601)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert "--nproc-per-node=4" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29601"
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "4", "--steps", "7", "--warmup", "2"]  # own flags forwarded, --dry-launch dropped


def test_cli_fails_loudly_without_enough_gpus_and_dry_launch_prints_the_command():
    # this container has no GPU: `--gpus 2` must exit non-zero and print NO result line
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True,
                       timeout=300, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    import torch

    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible: the request can be honoured here")
    assert p.returncode != 0 and p.stdout.strip() == "" and "--gpus 2 needs 2 visible GPUs" in p.stderr
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-launch", "--steps", "3"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0
    j = json.loads(p.stdout)
    assert j["dry_launch"] and j["n_gpus"] == 8 and "--nproc-per-node=8" in j["command"] and "--dry-launch" not in j["command"]


def test_kernel_families_cover_the_step_kernels():
    names = {
        "void mlp_fused_kernel<224, 2, 8, 4>(MlpArgs)": "mlp_fused",
        "_Z19gemm_tn_fast_kernelIDF16bLi256ELb1ELb0ELi64ELi1ELi128EEv7VsxGemm": "gemm_tn_fast",
        "_Z14gemm_tn_kernelIDF16bLi128ELb1EEv7VsxGemmi": "gemm_tn_generic",
        "void (anonymous namespace)::gemm_nt2_lnbwd_kernel<256>(VsxGemm)": "gemm_nt2",
        "void (anonymous namespace)::gemm_nt2_kernel<3, 256, false>(VsxGemm)": "gemm_nt2",
        "_Z19gemm_nt_fast_kernelIDF16bLi3ELb0ELi64ELi1ELi128EEv7VsxGemm": "gemm_nt_fast",
        "_Z14gemm_nt_kernelIDF16bLi128ELi128ELi2ELi2ELi32ELi2EEv7VsxGemm": "gemm_nt_generic",
        "_Z19dwconv7_mfma_kernelILi2ELb1EEvPKDF16bPKfS3_S1_PDF16biiiiiii": "dwconv7",
        "void dwconv7_wgrad_mfma_kernel<1>(...)": "dwconv7",
        "_Z20head_conv_fwd_kernelPKDF16bS0_PKfPDF16bPfS4_ii": "head",
        "_Z26head_out_bwd1_wgrad_kernelILi32ELi8EEv": "head",
        "void ssim_tile_fused_kernel<true>(float const*)": "loss",
        "_Z13ln_bwd_kernelIDF16bLi32ELi1ELb1EEv": "layernorm",
        "_Z19grn_q_reduce_kernelIDF16bEv": "grn_small",
        "__amd_rocclr_copyBuffer": "other",
    }
    for k, fam in names.items():
        assert bench.kernel_family(k) == fam, k
    # every family the live timer can emit for a wrapper is one the trace side knows
    trace_side = {f for _, f in bench.KERNEL_FAMILY}
    assert set(bench.OP_FAMILY.values()) <= trace_side


# ------------------------------------------------------------------ multi-rank helpers of the bench line
def _rank_logic_worker(rank, world, init_file, out_dir, diverge):
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    torch.manual_seed(0)
    flat = torch.randn(1000)
    if diverge and rank == 1:
        flat[123] += 1e-7 * flat[123].abs() + 1e-12  # one parameter, one ulp-sized step away: still a different checksum
    agree, fsum = bench.ranks_agree(flat)
    rt = bench.rank_times(0.010 * (rank + 1) * 5, 5, "cpu")  # rank r took 10 (r + 1) ms / step
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump({"agree": agree, "times": rt}, f)
    dist.destroy_process_group()


@pytest.mark.parametrize("diverge", [False, True])
def test_rank_consistency_and_rank_times_world2_gloo(tmp_path, diverge):
    """the two collectives the N > 1 bench line adds — the parameter checksum and the per-rank step times — with world size 2 on
    gloo: identical parameters agree, ONE element differing by an ulp does not, and every rank reports the same min / max"""
    import torch.multiprocessing as mp

    init_file = str(tmp_path / "init")
    mp.spawn(_rank_logic_worker, args=(2, init_file, str(tmp_path), diverge), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"r{i}.json")) for i in range(2)]
    assert r[0]["agree"] == r[1]["agree"] == (not diverge)
    assert r[0]["times"] == r[1]["times"]
    assert r[0]["times"]["per_rank"] == [10.0, 20.0] and r[0]["times"]["min"] == 10.0 and r[0]["times"]["max"] == 20.0


def _state_worker(rank, world, init_file, out_dir, reduce):
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    flat = torch.randn(1000, generator=torch.Generator().manual_seed(0))  # the same seeded parameters on every rank
    grad = torch.randn(1000, generator=torch.Generator().manual_seed(1 + rank))  # each rank's share from a batch of its own
    if reduce:
        dist.all_reduce(grad)
    m = 0.1 * grad  # AdamW's first moment after one step
    with open(os.path.join(out_dir, f"s{rank}.json"), "w") as f:
        json.dump({"agree": bench.training_state_agree(flat, grad, m)}, f)
    dist.destroy_process_group()


@pytest.mark.parametrize("reduce", [True, False])
def test_training_state_check_catches_a_missing_all_reduce_world2_gloo(tmp_path, reduce):
    """the parameters are identical on both ranks either way (learning rate 0 keeps them seeded): only the gradients and the
    moment show whether the all-reduce happened"""
    import torch.multiprocessing as mp

    mp.spawn(_state_worker, args=(2, str(tmp_path / "init"), str(tmp_path), reduce), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"s{i}.json")) for i in range(2)]
    assert r[0]["agree"] == r[1]["agree"] == reduce


def test_watchdog_names_rank_and_phase_and_exits_nonzero():
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench.Watchdog('first all-reduce', 0.5, 3):\n"
            "    time.sleep(30)\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 17 and "rank 3" in p.stderr and "first all-reduce" in p.stderr
    # a phase that finishes in time leaves no trace
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench.Watchdog('x', 30, 0):\n"
            "    pass\nprint('done')\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "done"


def test_mlp_mode_names_the_kernel_template():
    assert bench.mlp_mode("mlp_fc1_ln", {"store_h": False}) == 6 and bench.mlp_mode("mlp_fc1_ln", {}) == 2
    assert bench.mlp_mode("mlp_bwd_dh_ln", {}) == 7 and bench.mlp_mode("mlp_stats", {}) == 0
    assert bench.kernel_family("void mlp_fused_kernel_sf<224, 2, 8, 6>(MlpArgs)") == "mlp_fused"


# ------------------------------------------------------------------ --dump-outputs / --full
def test_dump_outputs_writes_float32_arrays_at_fixed_positions(tmp_path):
    """the files --dump-outputs writes: float32 .npy, the loss as shape [1], parameters and gradients sampled at the same seeded
    positions on every call (two builds dumped with the same arguments are compared element for element)"""
    import numpy as np
    import torch

    n, k = 10_000, 1_000
    flat, grad, loss = torch.arange(n, dtype=torch.float32), -torch.arange(n, dtype=torch.float32), torch.tensor(0.25)
    shapes = bench.dump_outputs(str(tmp_path / "a"), loss, flat, grad, sample=k)
    bench.dump_outputs(str(tmp_path / "b"), loss, flat.clone(), grad.clone(), sample=k)
    assert shapes == {"loss": [1], "params": [k], "grads": [k]}
    a = {nm: np.load(tmp_path / "a" / f"{nm}.npy") for nm in shapes}
    assert all(v.dtype == np.float32 for v in a.values()) and a["loss"][0] == 0.25
    idx = a["params"].astype(np.int64)
    assert len(np.unique(idx)) == k and np.all(np.diff(idx) > 0) and np.array_equal(a["grads"], -a["params"])
    for nm in shapes:
        assert np.array_equal(a[nm], np.load(tmp_path / "b" / f"{nm}.npy"))
    # a buffer no larger than the sample is written whole
    small = bench.dump_outputs(str(tmp_path / "c"), loss, flat[:50], grad[:50], sample=k)
    assert small["params"] == [50] and np.array_equal(np.load(tmp_path / "c" / "params.npy"), np.arange(50, dtype=np.float32))
    # the flagship's dump stays within 64 MB whatever the parameter count
    assert 4 * (1 + 2 * bench.DUMP_SAMPLE) <= 64 * 2**20


def test_full_and_dump_outputs_are_forwarded_to_the_ranks():
    cmd = bench.launch_command(2, ["--gpus", "2", "--steps", "4", "--full", "--dump-outputs", "out", "--dry-launch"], port=29602)
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "2", "--steps", "4", "--full", "--dump-outputs", "out"]
