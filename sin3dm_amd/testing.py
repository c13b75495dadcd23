"""Deterministic synthetic weights and inputs for parity tests, smoke() and bench.py.

There are no pretrained checkpoints offline, so every test, fixture and
benchmark runs on seeded synthetic parameters.  The generator is numpy PCG64 keyed by the
crc32 of the parameter *name*, so a tensor's values depend on nothing but (name, shape, seed):
the fixture generator (tests/golden/make_golden.py, which loads these into the *reference*
modules) and the GPU-box tests regenerate bit-identical weights without shipping them.

Parameter names/shapes restate the reference constructors:
  TriplaneUNetModelSmall.__init__   src/diffusion/unet_triplane.py:346-449
  TriplaneResBlock.__init__         src/diffusion/unet_triplane.py:194-262
  AutoEncoderGroupSkip.__init__     src/encoding/networks.py:124-149
  TriplaneGroupResnetBlock.__init__ src/encoding/blocks.py:190-235
  DecoderMLPSkipConcat.__init__     src/encoding/blocks.py:66-83
  AutoEncoderGroupPBR.__init__      src/encoding/networks.py:227-255
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np

PLANES = ("xy", "xz", "yz")


def _parse_mult(channel_mult):
    if isinstance(channel_mult, str):
        return tuple(int(c) for c in channel_mult.split(","))
    return tuple(int(c) for c in channel_mult)


def unet_param_shapes(in_channels=12, model_channels=64, out_channels=12, num_res_blocks=1,
                      channel_mult=(1, 2), use_scale_shift_norm=True, rollout=True):
    """name -> shape for TriplaneUNetModelSmall (rollout=True) / ...SmallRaw (rollout=False)."""
    channel_mult = _parse_mult(channel_mult)
    mc = model_channels
    ted = 4 * mc
    sh = OrderedDict()

    def lin(prefix, o, i):
        sh[prefix + ".weight"] = (o, i)
        sh[prefix + ".bias"] = (o,)

    def tconv(prefix, cin, cout, k, is_rollout):
        for p in PLANES:
            sh[f"{prefix}.conv_{p}.weight"] = (cout, cin * 3 if is_rollout else cin, k, k)
            sh[f"{prefix}.conv_{p}.bias"] = (cout,)

    def tnorm(prefix, c):
        for p in PLANES:
            sh[f"{prefix}.norm_{p}.weight"] = (c,)
            sh[f"{prefix}.norm_{p}.bias"] = (c,)

    def resblock(prefix, c, cout):
        tnorm(prefix + ".in_layers.0", c)
        tconv(prefix + ".in_layers.2", c, cout, 3, rollout)
        lin(prefix + ".emb_layers.1", 2 * cout if use_scale_shift_norm else cout, ted)
        tnorm(prefix + ".out_layers.0", cout)
        tconv(prefix + ".out_layers.2", cout, cout, 3, rollout)
        if c != cout:
            tconv(prefix + ".skip_connection", c, cout, 1, False)

    lin("time_embed.0", ted, mc)
    lin("time_embed.2", ted, ted)
    ch = input_ch = int(channel_mult[0] * mc)
    tconv("in_conv.0", in_channels, ch, 1, False)
    # The reference updates `ch` once per level and appends one skip width per level while the
    # decoder pops one per res block (unet_triplane.py:383-419): num_res_blocks != 1 cannot even be
    # constructed there (IndexError on input_block_chans.pop()), so only 1 is a valid topology.
    if num_res_blocks != 1:
        raise NotImplementedError("reference topology is only constructible with num_res_blocks=1")
    chans = [ch]
    for level, mult in enumerate(channel_mult):
        idx = 0 if level == 0 else 1  # a parameter-free Downsample sits at index 0
        resblock(f"input_blocks.{level}.{idx}", ch, int(mult * mc))
        ch = int(mult * mc)
        chans.append(ch)
    nlev = len(channel_mult)
    for oi, (level, mult) in enumerate(list(enumerate(channel_mult))[::-1]):
        for i in range(num_res_blocks):
            ich = chans.pop()
            if level == nlev - 1 and i == 0:
                ich = 0
            resblock(f"output_blocks.{oi}.{i}", ch + ich, int(mc * mult))
        ch = int(mc * mult)
    tnorm("out.0", ch)
    tconv("out.2", input_ch, out_channels, 1, False)
    return sh


def ae_param_shapes(geo_feat_channels=4, tex_feat_channels=8, feat_channel_up=64,
                    mlp_hidden_channels=256, mlp_hidden_layers=4, tex_channels=3, with_encoder=False):
    """name -> shape for AutoEncoderGroupSkip: the decode side, plus the two Conv3d encoders when with_encoder."""
    sh = OrderedDict()
    up, hid = feat_channel_up, mlp_hidden_channels
    if with_encoder:
        sh["geo_encoder.weight"] = (geo_feat_channels, 1, 4, 4, 4)
        sh["geo_encoder.bias"] = (geo_feat_channels,)
        sh["tex_encoder.weight"] = (tex_feat_channels, tex_channels + 1, 4, 4, 4)
        sh["tex_encoder.bias"] = (tex_feat_channels,)

    def block(prefix, cin):
        sh[prefix + ".in_layers.0.weight"] = (3 * up, cin, 5, 5)
        sh[prefix + ".in_layers.0.bias"] = (3 * up,)
        for p in PLANES:
            sh[f"{prefix}.norm_{p}.weight"] = (up,)
            sh[f"{prefix}.norm_{p}.bias"] = (up,)
        sh[prefix + ".out_layers.1.weight"] = (3 * up, up, 5, 5)
        sh[prefix + ".out_layers.1.bias"] = (3 * up,)
        sh[prefix + ".shortcut.weight"] = (3 * up, cin, 1, 1)
        sh[prefix + ".shortcut.bias"] = (3 * up,)

    def mlp(prefix, cin, cout):
        n = mlp_hidden_layers // 2
        sh[f"{prefix}.first_layers.0.weight"] = (hid, cin)
        sh[f"{prefix}.first_layers.0.bias"] = (hid,)
        for i in range(n):
            sh[f"{prefix}.first_layers.{2 * (i + 1)}.weight"] = (hid, hid)
            sh[f"{prefix}.first_layers.{2 * (i + 1)}.bias"] = (hid,)
        sh[f"{prefix}.second_layers.0.weight"] = (hid, cin + hid)
        sh[f"{prefix}.second_layers.0.bias"] = (hid,)
        for i in range(n - 1):
            sh[f"{prefix}.second_layers.{2 * (i + 1)}.weight"] = (hid, hid)
            sh[f"{prefix}.second_layers.{2 * (i + 1)}.bias"] = (hid,)
        sh[f"{prefix}.second_layers.{2 * n}.weight"] = (cout, hid)
        sh[f"{prefix}.second_layers.{2 * n}.bias"] = (cout,)

    block("geo_convs", geo_feat_channels)
    mlp("geo_decoder", up, 1)
    block("tex_convs", tex_feat_channels)
    mlp("tex_decoder", up, tex_channels)
    return sh


def geo_only_param_shapes(geo_feat_channels=4, feat_channel_up=64, mlp_hidden_channels=256, mlp_hidden_layers=4,
                          with_encoder=False):
    """name -> shape for AutoEncoderGroupSkip / AutoEncoderGroupPBR with use_tex=False (data_type sdf): the geo side of
    ae_param_shapes, which is the same network in both."""
    full = ae_param_shapes(geo_feat_channels, 1, feat_channel_up, mlp_hidden_channels, mlp_hidden_layers, 1, with_encoder)
    return OrderedDict((k, v) for k, v in full.items() if k.startswith("geo_"))


def pbr_param_shapes(geo_feat_channels=4, tex_feat_channels=8, feat_channel_up=64, mlp_hidden_channels=256,
                     mlp_hidden_layers=4, tex_channels=8, use_tex=True, with_encoder=False):
    """name -> shape for AutoEncoderGroupPBR (src/encoding/networks.py:227-255) in state_dict order: the geo side of the skip
    net; tex_convs = two 3x3 TriplaneGroupResnetBlocks, the second without shortcut parameters and with its conv at
    in_layers.1 (a SiLU sits at index 0); the rgb / mr / normal DecoderMLPSkipConcat heads."""
    if not use_tex:
        return geo_only_param_shapes(geo_feat_channels, feat_channel_up, mlp_hidden_channels, mlp_hidden_layers, with_encoder)
    up = feat_channel_up
    skip = ae_param_shapes(geo_feat_channels, tex_feat_channels, up, mlp_hidden_channels, mlp_hidden_layers, tex_channels,
                           with_encoder)
    sh = OrderedDict((k, v) for k, v in skip.items() if k.startswith(("geo_", "tex_encoder")))

    def block(prefix, cin, conv_idx, shortcut):
        sh[f"{prefix}.in_layers.{conv_idx}.weight"] = (3 * up, cin, 3, 3)
        sh[f"{prefix}.in_layers.{conv_idx}.bias"] = (3 * up,)
        for p in PLANES:
            sh[f"{prefix}.norm_{p}.weight"] = (up,)
            sh[f"{prefix}.norm_{p}.bias"] = (up,)
        sh[prefix + ".out_layers.1.weight"] = (3 * up, up, 3, 3)
        sh[prefix + ".out_layers.1.bias"] = (3 * up,)
        if shortcut:
            sh[prefix + ".shortcut.weight"] = (3 * up, cin, 1, 1)
            sh[prefix + ".shortcut.bias"] = (3 * up,)

    block("tex_convs.0", tex_feat_channels, 0, True)
    block("tex_convs.1", up, 1, False)
    for head, cout in (("rgb_decoder", 3), ("mr_decoder", 2), ("normal_decoder", 3)):
        one = ae_param_shapes(1, 1, up, mlp_hidden_channels, mlp_hidden_layers, cout)
        for k, v in one.items():
            if k.startswith("tex_decoder."):
                sh[head + k[len("tex_decoder"):]] = v
    return sh


def synthetic_tensor(name, shape, seed=0):
    """fp32 array for parameter `name`: fan-in scaled weights, small biases, GN gains near 1."""
    rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
    x = rng.standard_normal(size=shape)
    leaf = name.rsplit(".", 1)[-1]
    is_norm = ".norm_" in name
    if is_norm and leaf == "weight":
        x = 1.0 + 0.2 * x
    elif leaf == "bias":
        x = 0.1 * x
    else:
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        x = x * (1.0 / np.sqrt(fan_in))
        if "emb_layers" in name or "time_embed" in name:
            x = x * 1.5
    return np.ascontiguousarray(x.astype(np.float32))


def synthetic_state_dict(shapes, seed=0, as_torch=True):
    out = OrderedDict()
    for name, shape in shapes.items():
        a = synthetic_tensor(name, shape, seed)
        if as_torch:
            import torch
            a = torch.from_numpy(a)
        out[name] = a
    return out


def synthetic_noise(shape, seed):
    """Seeded N(0,1) fp32 array (used where a fixture does not store the noise explicitly)."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xA11CE]))
    return np.ascontiguousarray(rng.standard_normal(size=shape).astype(np.float32))


class TorchCpuStreamModel:
    """Host model of torch's float32 CPU noise stream on numpy's MT19937: what the tests hold the device kernels of
    diffusion/cpu_stream.py and the recorded torch draws against.  A test helper, not a product path.
    seed=k is the stream after `torch.manual_seed(k)`; key / pos continue a parsed generator state."""

    def __init__(self, seed=None, key=None, pos=None):
        self.mt = np.random.MT19937()
        if key is not None:
            self.mt.state = {"bit_generator": "MT19937", "state": {"key": np.asarray(key, dtype=np.uint32), "pos": int(pos)}}
        else:
            self.mt._legacy_seeding(int(seed) & 0xFFFFFFFF)
        self.words = 0                      # 32-bit words consumed so far

    def state(self):
        s = self.mt.state["state"]
        return np.asarray(s["key"], dtype=np.uint32), int(s["pos"])

    def rand(self, n):
        self.words += int(n)
        r = self.mt.random_raw(int(n)).astype(np.uint32)
        return (r & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)

    @staticmethod
    def _box_muller(u):
        """rows of 16 uniforms -> rows of 16 normals: columns j and j + 8 are one pair"""
        u1, u2 = np.float32(1) - u[:, :8], u[:, 8:]
        rad = np.sqrt(np.float32(-2) * np.log(u1))
        th = np.float32(2 * np.pi) * u2
        return np.concatenate([rad * np.cos(th), rad * np.sin(th)], 1).astype(np.float32)

    def randn(self, n):
        n = int(n)
        assert n >= 16, "torch draws fewer than 16 elements through another path"
        d = self.rand(n)
        m = n - n % 16
        d[:m] = self._box_muller(d[:m].reshape(-1, 16)).ravel()
        if n % 16:
            d[n - 16:] = self._box_muller(self.rand(16).reshape(1, 16)).ravel()      # the last 16 are redrawn from 16 more words
        return d


def gyroid_sdf(shape, freq=2.0, phase=(0.0, 0.0, 0.0), thickness=0.35):
    """A thickened gyroid |sin x cos y + sin y cos z + sin z cos x| - thickness on a grid of `shape` voxels (float32, negative
    inside): `freq` periods along the longest axis, `phase` shifts it per axis.  A procedural stand-in for an SDF grid with many
    near-surface patches, for the evaluation tests, their fixture generator and tools/bench_eval.py."""
    n = float(max(shape))
    x, y, z = (2.0 * np.pi * freq * (np.arange(s, dtype=np.float64) + 0.5) / n + p for s, p in zip(shape, phase))
    x, y, z = x[:, None, None], y[None, :, None], z[None, None, :]
    g = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x)
    return np.ascontiguousarray((np.abs(g) - thickness).astype(np.float32))
