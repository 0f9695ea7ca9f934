"""Writes tests/golden/aux_heads.pt: what the reference's embedding-space heads give on the case tables of
tests/ref_aux_heads.py.

    python tools/gen_golden_aux_heads.py <checkout of the reference>/packages/viscy-models/src/viscy_models/components/heads.py

The reference module is loaded by path.  What it imports beyond torch and does not need for these heads (``monai.*``,
``viscy_models.components.blocks``) is stubbed here; ``viscy_models.schedule.cosine_anneal`` is the few lines below.  Inputs are
not stored: the tables rebuild them from seeds and shapes.  Per kernel case: the reference classifier's logits checksum, loss,
top-1 / top-k and sampled gradients in fp32 and fp64.  Per head case: loss, accuracies, sampled input / parameter gradients and
the buffers after one training forward.  Also the state-dict keys for ``hidden_dims`` 256 and [64, 32], the constructor
signatures, and the OPS head's weight schedule."""
import importlib.util
import inspect
import math
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_aux_heads as RA  # noqa: E402


def _cosine_anneal(start, end, epoch, warmup_epochs):
    if epoch >= warmup_epochs:
        return end
    return end + (start - end) * 0.5 * (1.0 + math.cos(math.pi * epoch / warmup_epochs))


def load_reference(path):
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        mod.__path__ = []
        sys.modules[name] = mod

    stub("monai")
    stub("monai.networks")
    stub("monai.networks.blocks", Convolution=None, UpSample=None)
    stub("monai.networks.utils", normal_init=None)
    stub("viscy_models")
    stub("viscy_models.components")
    stub("viscy_models.components.blocks", icnr_init=None)
    stub("viscy_models.schedule", cosine_anneal=_cosine_anneal)
    spec = importlib.util.spec_from_file_location("reference_heads", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_kernel_case(ref, inp, dtype):
    """the reference's classifier module holding the case's tensors, its cross-entropy and ``log_metrics`` arithmetic"""
    C, H = inp["W"].shape
    if inp["mode"] == "cosine":
        clf = ref.CosineClassifier(H, C)
        clf.log_scale.data = inp["log_scale"].clone()
    else:
        clf = torch.nn.Linear(H, C)
        clf.bias.data = inp["bias"].clone()
    clf.weight.data = inp["W"].clone()
    clf = clf.to(dtype)
    h = inp["h"].to(dtype).clone().requires_grad_(True)
    logits = clf(h)
    loss = F.cross_entropy(logits, inp["y"])
    (loss * RA.GOUT).backward()
    y, k = inp["y"], inp["k"]
    top1 = (logits.argmax(dim=1) == y).float().mean()
    topk = (logits.topk(k, dim=1).indices == y.unsqueeze(1)).any(dim=1).float().mean()
    grads = {"dh": h.grad, "dW": clf.weight.grad}
    grads["dlog_scale" if inp["mode"] == "cosine" else "dbias"] = (clf.log_scale if inp["mode"] == "cosine" else clf.bias).grad
    return dict(loss=float(loss), top1=float(top1), topk=float(topk), checksum=float(logits.detach().double().sum()),
                abs_checksum=float(logits.detach().double().abs().sum()),
                **{n: g.reshape(-1)[RA.grad_sample_index(g.numel())].clone() for n, g in grads.items()})


def run_head_case(ref, name, dtype):
    case = RA.build_head_case(name, cls=ref.ClassificationHead)
    head = case["head"].to(dtype)
    x = case["x"].to(dtype).clone().requires_grad_(True)
    logits = head(x)
    loss = head.compute_loss(logits, case["y"])
    (loss * RA.GOUT).backward()
    logged = {}
    head.log_metrics({"loss": loss.detach(), "logits": logits.detach(), "y": case["y"]}, lambda key, v: logged.update({key: float(v)}),
                     "train")
    pick = lambda t: t.reshape(-1)[RA.grad_sample_index(t.numel())].clone()  # noqa: E731
    return dict(loss=float(loss), logged=logged, dx=pick(x.grad),
                grads={n: pick(p.grad) for n, p in head.named_parameters()},
                buffers={n: pick(b.detach()) for n, b in head.named_buffers()})


def signature(cls):
    return [(n, None if p.default is inspect.Parameter.empty else repr(p.default))
            for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]


def main():
    ref = load_reference(sys.argv[1])
    out = {"kernel": {}, "head": {}, "torch": str(torch.__version__)}
    for name in RA.KERNEL_CASES:
        inp = RA.build_kernel_case(name)
        out["kernel"][name] = {"fp32": run_kernel_case(ref, inp, torch.float32), "fp64": run_kernel_case(ref, inp, torch.float64)}
        a, b = out["kernel"][name]["fp32"], out["kernel"][name]["fp64"]
        print(f"{name:28s} loss {float(b['loss']):.6f}  fp32 rel err {abs(float(a['loss']) - float(b['loss'])) / max(abs(float(b['loss'])), 1e-300):.1e}"
              f"  top1 {float(b['top1']):.3f} top{inp['k']} {float(b['topk']):.3f}")
    for name in RA.HEAD_CASES:
        out["head"][name] = {"fp32": run_head_case(ref, name, torch.float32), "fp64": run_head_case(ref, name, torch.float64)}
        print(f"{name:28s} loss {float(out['head'][name]['fp64']['loss']):.6f}")
    out["state_dict_keys"] = {
        "256": list(ref.ClassificationHead("h", "k", 8, 256, 3).state_dict()),
        "[64, 32]": list(ref.ClassificationHead("h", "k", 8, [64, 32], 3, cosine_classifier=False).state_dict()),
    }
    out["signatures"] = {n: signature(getattr(ref, n)) for n in ("BaseHead", "ClassificationHead", "CosineClassifier", "MLP")}
    head = ref.ClassificationHead(**RA.OPS_HEAD)
    sched = {"initial": head.get_weight()}
    for e in RA.SCHEDULE_EPOCHS:
        head.step(e)
        sched[e] = head.get_weight()
    out["ops_schedule"] = sched
    out["package_exports"] = ["BaseHead", "ClassificationHead"]  # what viscy_models/components/__init__.py re-exports of these
    path = os.path.join(ROOT, "tests", "golden", "aux_heads.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
