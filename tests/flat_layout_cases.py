"""The model configurations whose flat parameter layout tests/golden/flat_layout.json pins, and the record taken of each.
Shared by tests/test_flat_cpu.py and tools/gen_golden_flat_layout.py.  Optimiser state (Adam's m, v) is indexed by flat offset,
so the layout is a checkpoint format: engines construct on the CPU with the torch-stated ops, the constructor launches nothing."""

import hashlib

from tests import ref_ops, ref_ops_fnet3d

_FCMAE_SMALL = dict(encoder_blocks=[1, 1, 1, 1], dims=[96, 192, 384, 768], decoder_conv_blocks=1)
_EMBED = dict(in_channels=1, in_stack_depth=5, embedding_dim=32, projection_dim=16, depths=(1, 1, 2, 1), dims=(16, 32, 64, 128))


def _unext2(kw):
    from viscy_amd.unext2 import UNeXt2

    return UNeXt2(**kw), ref_ops


def _fcmae(kw):
    from viscy_amd.fcmae import FullyConvolutionalMAE

    return FullyConvolutionalMAE(**kw)._core, ref_ops


def _embed(backbone):
    from viscy_amd.contrastive import ContrastiveEncoder

    return ContrastiveEncoder(backbone, **_EMBED)._core, ref_ops


def _fnet3d(kw):
    from viscy_amd.unet3d import Unet3d

    return Unet3d(**kw), ref_ops_fnet3d


def _cases():
    from tests.test_schedule_cpu import CASES

    c = {f"unext2_{tag}": (_unext2, kw) for tag, kw, _ in CASES}
    c["fcmae"] = (_fcmae, dict(in_channels=2, out_channels=2, encoder_blocks=[1, 1, 2, 1], dims=[16, 32, 64, 128],
                               decoder_conv_blocks=1, stem_kernel_size=(5, 4, 4), in_stack_depth=5))
    # 2x2 stem: the last decoder stage has out_channels * in_stack_depth * 4 = 8 channels (the narrow family)
    c["fcmae_2x2_c8"] = (_fcmae, dict(_FCMAE_SMALL, in_channels=1, out_channels=2, stem_kernel_size=(1, 2, 2), in_stack_depth=1,
                                      pretraining=False))
    c["embed_convnext_tiny"] = (_embed, "convnext_tiny")
    c["embed_convnextv2_tiny"] = (_embed, "convnextv2_tiny")
    c["fnet3d_d2_m4_out1"] = (_fnet3d, dict(in_channels=1, out_channels=1, depth=2, mult_chan=4))
    c["fnet3d_d3_m2_out2"] = (_fnet3d, dict(in_channels=1, out_channels=2, depth=3, mult_chan=2))
    c["fnet3d_d1"] = (_fnet3d, dict(in_channels=1, out_channels=1, depth=1, mult_chan=4))
    return c


FROZEN_CASE = "unext2_femto_preconv"  # also recorded with encoder + stem frozen (the FCMAE fine-tuning recipe's pattern)


def tags():
    return list(_cases())


def make(tag):
    """-> (core module, ops) of configuration ``tag``, on the CPU; ``core.engine(ops)`` is the engine"""
    fn, arg = _cases()[tag]
    return fn(arg)


def record(tag, core, eng):
    name_of = {id(p): n for n, p in core.named_parameters()}
    names = [name_of[id(p)] for p in eng.order]
    rec = dict(n_params=len(names), names_sha256=hashlib.sha256("\n".join(names).encode()).hexdigest(),
               offsets=[int(o) for o in eng.offsets], bucket_bounds=[[int(lo), int(hi)] for lo, hi in eng.bucket_bounds],
               flat_numel=int(eng.flat.numel()), trainable_numel=int(eng.trainable_numel()))
    if tag == FROZEN_CASE:
        core.encoder_stages.requires_grad_(False)
        core.stem.requires_grad_(False)
        rec["trainable_numel_encoder_frozen"] = int(eng.trainable_numel())
    return rec
