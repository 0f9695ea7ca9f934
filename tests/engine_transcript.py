"""TEST INFRASTRUCTURE — the launch transcript of ``viscy_amd.engine_unext2.Engine``: a recorder that wraps every public
function of an ops module in place (the module object stays the same, so ``Engine._hip`` keeps its value) and notes, for every
top-level call, the function's name and a description of each argument, and the table of cases whose transcript
tests/golden/engine_transcript.json pins.  Shared by tests/test_engine_transcript_cpu.py, tools/gen_golden_engine_transcript.py
and the parent-against-head comparisons on the GPU (profiles/engine_layers_refactor.txt).

A launch is one string, ``name(arg, ..., key=arg)``, in a normal form (``Recorder._note_call``).  A tensor is ``dtype[shape]``; a view into the engine's flat parameter /
gradient buffer is ``p@offset:[shape]`` / ``g@offset:[shape]`` (which parameter a launch reads, which gradient slot it writes).
Scalars, strings, None and lists / tuples of them stand by value (floats by ``repr``), dtypes by name.  Calls made by an ops
function itself are not recorded.  The bucket indices ``backward_stages`` yields are recorded as ``yield(k)``."""

import inspect

import torch

from tests import flat_layout_cases, ref_ops, ref_ops_narrow

_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64", torch.int32: "i32", torch.int64: "i64",
       torch.uint8: "u8", torch.bool: "bool", torch.float16: "f16"}


class Recorder:
    def __init__(self, ops, eng):
        self.ops, self.eng, self.log, self._depth, self._saved = ops, eng, [], 0, {}

    def _arg(self, a):
        if isinstance(a, torch.Tensor):
            shape = str(list(a.shape)).replace(" ", "")
            if a.numel():
                for tag, buf in (("p", self.eng.flat), ("g", self.eng.flat_grad)):
                    if a.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr():
                        return f"{tag}@{a.storage_offset()}:{shape}"
            return _DT.get(a.dtype, str(a.dtype)) + shape
        if isinstance(a, torch.dtype):
            return _DT.get(a, str(a))
        if isinstance(a, (list, tuple)):
            return "[" + ",".join(self._arg(v) for v in a) + "]"
        if a is None or isinstance(a, (bool, int, str)):
            return str(a)
        if isinstance(a, float):
            return repr(a)
        return f"<{type(a).__name__}>"  # a device, a saved-state tuple of a loss: not an engine argument

    def note(self, name, *args, **kw):
        parts = [self._arg(a) for a in args] + [f"{k}={self._arg(v)}" for k, v in kw.items()]
        self.log.append(f"{name}({','.join(parts)})")

    def _note_call(self, name, sig, args, kw):
        """the call in normal form: parameters in the order of the signature, one without a default by value, one with a default
        as ``name=value`` and only where the value is not the default — so neither the order of keywords nor spelling out a
        default is a difference"""
        bound = sig.bind(*args, **kw).arguments
        parts = []
        for pname, p in sig.parameters.items():
            if pname not in bound:
                continue
            v = bound[pname]
            if p.kind is p.VAR_POSITIONAL:
                parts += [self._arg(a) for a in v]
            elif p.kind is p.VAR_KEYWORD:
                parts += [f"{k}={self._arg(a)}" for k, a in sorted(v.items())]
            elif p.default is p.empty:
                parts.append(self._arg(v))
            elif isinstance(v, torch.Tensor) or type(v) is not type(p.default) or v != p.default:
                parts.append(f"{pname}={self._arg(v)}")
        self.log.append(f"{name}({','.join(parts)})")

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*args, **kw):
            if self._depth == 0:
                self._note_call(name, sig, args, kw)
            self._depth += 1
            try:
                return fn(*args, **kw)
            finally:
                self._depth -= 1

        return wrapped

    def __enter__(self):
        for name, fn in list(vars(self.ops).items()):
            own = getattr(fn, "__module__", "") in (self.ops.__name__, ref_ops.__name__)
            if inspect.isfunction(fn) and own and not name.startswith("_"):
                self._saved[name] = fn
                setattr(self.ops, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.ops, name, fn)
        self._saved = {}

    def take(self):
        log, self.log = self.log, []
        return log


# ------------------------------------------------------------------------------------------------ the cases
def _hw(h, w, B=2):
    return lambda core: (B, core.cfg["in_channels"], core.cfg["in_stack_depth"], h, w)


def _masks(core, shape):
    """the row maps of a seeded mask at ratio 0.5 on the stride-32 grid (viscy_amd.fcmae.generate_mask's draw)"""
    from viscy_amd.fcmae import generate_mask, stage_row_maps

    torch.manual_seed(5)
    low = generate_mask(shape, 32, 0.5, "cpu")
    kept = int((~low).flatten(1).sum(1)[0])
    s = core.cfg["stem_kernel"][-1]
    H, W = shape[-2] // s, shape[-1] // s
    return [tuple(t.to(core_device(core)) if isinstance(t, torch.Tensor) else t for t in m)
            for m in stage_row_maps(~low, [(H >> i, W >> i) for i in range(4)], kept)]


def core_device(core):
    return next(core.parameters()).device


def _freeze(core):
    core.encoder_stages.requires_grad_(False)
    core.stem.requires_grad_(False)


def _droppath(kw):
    from viscy_amd.unext2 import UNeXt2

    return UNeXt2(**kw, drop_path_rate=0.5), ref_ops


def _unext2_kw(tag):
    from tests.test_schedule_cpu import CASES

    return next(kw for t, kw, _ in CASES if t == tag)


# tag -> dict(model = tag of tests/flat_layout_cases.py (or a maker), shape(core) -> input shape, and what differs from a
# dense training step: masked, z1 (a Z = 1 input), bn_groups, frozen, inject (stochastic depth scales), need_bwd)
CASES = {
    "unext2_atto_pool": dict(model="unext2_atto_pool", shape=_hw(64, 96)),
    "unext2_femto_z15": dict(model="unext2_femto_z15", shape=_hw(64, 64)),
    "unext2_femto_preconv": dict(model="unext2_femto_preconv", shape=_hw(64, 96)),
    "fcmae_dense": dict(model="fcmae", shape=_hw(64, 64)),
    "fcmae_masked": dict(model="fcmae", shape=_hw(64, 64), masked=True),
    "fcmae_z1": dict(model="fcmae", shape=_hw(64, 64), z1=True),
    "fcmae_2x2_c8": dict(model="fcmae_2x2_c8", shape=_hw(32, 32), ops=ref_ops_narrow),
    "embed_convnext_tiny_g1": dict(model="embed_convnext_tiny", shape=_hw(64, 64, 4), bn_groups=1),
    "embed_convnext_tiny_g2": dict(model="embed_convnext_tiny", shape=_hw(64, 64, 4), bn_groups=2),
    "embed_convnextv2_tiny_g1": dict(model="embed_convnextv2_tiny", shape=_hw(64, 64, 4), bn_groups=1),
    "embed_convnextv2_tiny_g2": dict(model="embed_convnextv2_tiny", shape=_hw(64, 64, 4), bn_groups=2),
    "unext2_femto_preconv_frozen": dict(model="unext2_femto_preconv", shape=_hw(64, 96), frozen=True),
    "unext2_atto_droppath": dict(model=lambda: _droppath(_unext2_kw("atto_pool")), shape=_hw(64, 96), inject=True),
    "unext2_atto_infer": dict(model="unext2_atto_pool", shape=_hw(64, 96), need_bwd=False),
    # bf16 operands on the torch-stated ops: the stem's K = 80 is padded to 96, behind the `flush` of the weight task list.
    # The engine's two other `flush` calls (in front of `head_conv_dgrad_prep`: bf16 with need_bwd, c3 = 8, cmid = 32; in the
    # per-sample-weights fc2 branch of `_block_fwd`) are reached by no case of this table
    "unext2_atto_infer_bf16": dict(model="unext2_atto_pool", shape=_hw(64, 96), need_bwd=False, dt=torch.bfloat16),
}


def build(tag, device="cpu", ops=None, seed=0, shape=None):
    """-> (engine, step): ``step(rec)`` runs one forward (+ backward) of case ``tag`` and returns (out, engine); weights and
    inputs are seeded.  ``ops``: the backend instead of the case's torch-stated one; ``shape``: (B, H, W) instead of the
    case's."""
    case = CASES[tag]
    torch.manual_seed(seed)
    core, case_ops = flat_layout_cases.make(case["model"]) if isinstance(case["model"], str) else case["model"]()
    ops = case.get("ops", case_ops) if ops is None else ops
    core = core.to(device).train()
    if case.get("frozen"):
        _freeze(core)
    eng = core.engine(ops)
    xs = list(case["shape"](core))
    if shape is not None:
        xs[0], xs[3], xs[4] = shape
    if case.get("z1"):
        xs[2] = 1
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(xs, generator=gen).to(device)
    fwd = {}
    if case.get("masked"):
        fwd["masks"] = _masks(core, xs)
    if "bn_groups" in case:
        fwd["bn_groups"] = case["bn_groups"]
    n_dp = sum(1 for r in core.cfg.get("drop_path") or () if r > 0)

    def step(rec, dt=case.get("dt", torch.float32)):
        if case.get("inject"):  # one sample's branch dropped, the other scaled by 1 / keep, in every block that has a rate
            eng._dp_inject = [torch.tensor([2.0, 0.0] * (xs[0] // 2), device=device) for _ in range(n_dp)]
        with torch.no_grad():
            out, sv = eng.forward(x, dt, case.get("need_bwd", True), **fwd)
            if sv is None:
                rec.note("saved", None)
                return out
            outs = out if isinstance(out, tuple) else (out,)
            douts = tuple(torch.randn(o.shape, generator=gen).to(device) for o in outs)
            eng.reset_pending()  # backward_stages is driven from here
            for k in eng.backward_stages(sv, douts if len(douts) > 1 else douts[0]):
                rec.note("yield", k)
        return out

    return eng, step


def run_case(tag, steps=2, **kw):
    """the record of case ``tag``: the transcript of each of ``steps`` consecutive steps, and the arena sizes after the last"""
    eng, step = build(tag, **kw)
    out = []
    with Recorder(eng.ops, eng) as rec:
        for _ in range(steps):
            step(rec)
            out.append(rec.take())
    return dict(steps=out, za_need={str(k): int(v) for k, v in sorted(eng._za_need.items(), key=str)})


def pack(records):
    """{tag: run_case(tag)} -> the golden's form: every distinct launch string once (the two steps of a case, and the cases
    that share a model, repeat most of them), the transcripts as indices into that table"""
    table = {}
    cases = {tag: dict(steps=[[table.setdefault(s, len(table)) for s in step] for step in r["steps"]], za_need=r["za_need"])
             for tag, r in records.items()}
    return dict(launches=list(table), cases=cases)


def unpack(golden):
    table = golden["launches"]
    return {tag: dict(steps=[[table[i] for i in step] for step in r["steps"]], za_need=r["za_need"])
            for tag, r in golden["cases"].items()}


def first_difference(want, got):
    """None, or a message naming the first launch at which two transcripts differ"""
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return f"launch {i}:\n  golden {a}\n  now    {b}"
    if len(want) != len(got):
        i = min(len(want), len(got))
        extra = (want[i:i + 1] or got[i:i + 1])[0]
        return f"{len(want)} launches in the golden, {len(got)} now; launch {i} {'is missing' if len(want) > len(got) else 'is new'}: {extra}"
    return None
