"""AutoEncoderGroupSkip and AutoEncoderGroupPBR with the reference's constructors, parameter names and `decode` signature
(src/encoding/networks.py:124-225, 227-316) — decode runs in libsin3dm_hip.so.

The decode side covers the reference's three data types: sdftex (skip net, 1+3 columns), sdf (use_tex=False: the geo network
alone, 1 column, feature maps of fdim_geo channels) and sdfpbr (skip net with 8 sigmoid channels, or the PBR net: sdf | rgb 3 |
metallic-roughness 2 | normal 3, no sigmoid).  The training tier below is built for the skip net with 1..8 texture channels
(sdftex, and sdfpbr with --enc_net_type skip), for the geometry-only net of either class (sdf) and for the PBR net with its three
material heads (sdfpbr with --enc_net_type pbr).  The sdftex net has it from construction; the others keep their earlier
decode-only contract (`encode`, `forward`, `loss_and_grads` raise NotImplementedError) until `build_training_tier()` is called —
for the PBR net with texture `build_training_tier(material_heads=True)` —, which ShapeAutoEncoder does for training.

`decode(x, feat_maps, aabb)` keeps the reference semantics (sdf, sigmoid(rgb)); the per-plane conv blocks are
evaluated once per distinct triplane and cached (the reference recomputes them on every call with identical
results).

Training tier: `encode(vol)`, `forward(vol, x)` and `loss_and_grads(...)` run on the s3d_ae_*
entry points.  The parameters are then views of one flat device vector laid out [geo group | tex group] (the reference's
two AdamW parameter groups, :146-150; the geometry-only net has the geo group alone and `tex_group_begin` is the vector's
size); the input volume (1 + tex_channels channels, 1 for sdf) is reduced once to three 2-D projections (`set_volume`),
which is all the Conv3d-then-mean encoder needs.  The texture loss of 8 channels is the reference's three means (rgb, mr,
normal; model.py:226-233), of any other width one mean.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from ..diffusion.unet_triplane import _register
from ..testing import ae_param_shapes, geo_only_param_shapes, pbr_param_shapes


def get_networks(cfg):
    """Reference: src/encoding/networks.py:7-18."""
    use_tex = cfg.data_type != "sdf"
    tex_channels = 8 if cfg.data_type == "sdfpbr" else 3
    args = (cfg.fdim_geo, cfg.fdim_tex, cfg.fdim_up, cfg.hidden_dim, cfg.n_hidden_layers)
    if cfg.enc_net_type == "skip":
        return AutoEncoderGroupSkip(*args, use_tex=use_tex, tex_channels=tex_channels)
    if cfg.enc_net_type == "pbr":
        if cfg.data_type == "sdftex":
            # its decode has 8 material columns whatever tex_channels says: the reference can neither train (3-channel targets
            # against 8 outputs) nor export this pair
            raise ValueError("--enc_net_type pbr with --data_type sdftex: the PBR network decodes albedo, metallic, roughness "
                             "and normal (8 channels); use --data_type sdfpbr (or sdf), or --enc_net_type skip")
        return AutoEncoderGroupPBR(*args, use_tex=use_tex, tex_channels=tex_channels)
    if cfg.enc_net_type == "base":
        raise NotImplementedError("--enc_net_type base (AutoEncoderGroupV3) is not built: skip and pbr are")
    raise ValueError("Unknown net type: {}".format(cfg.enc_net_type))


class AutoEncoderGroupSkip(nn.Module):
    def __init__(self, geo_feat_channels, tex_feat_channels, feat_channel_up, mlp_hidden_channels, mlp_hidden_layers,
                 use_tex=True, tex_channels=3, posenc=0):
        super().__init__()
        if posenc:
            raise NotImplementedError("posenc>0 is not built")
        self.use_tex = bool(use_tex)
        self.geo_feat_dim = geo_feat_channels
        self.tex_feat_dim = tex_feat_channels
        self.cfg = (geo_feat_channels, tex_feat_channels, feat_channel_up, mlp_hidden_channels, mlp_hidden_layers,
                    tex_channels)
        # s3d_decoder_create_variant: 0 this net with texture, 1 geometry only, 2 the PBR net
        self.variant = self._TEX_VARIANT if self.use_tex else 1
        self.out_channels = {0: 1 + tex_channels, 1: 1, 2: 9}[self.variant]
        self.in_feat_channels = geo_feat_channels + (tex_feat_channels if self.use_tex else 0)
        shapes = dict(self._decode_shapes())
        # encoder parameters exist in the reference's checkpoints (ckpt_final.pth['net']); kept so they load
        enc = {"geo_encoder.weight": (geo_feat_channels, 1, 4, 4, 4), "geo_encoder.bias": (geo_feat_channels,)}
        if self.use_tex:
            enc.update({"tex_encoder.weight": (tex_feat_channels, tex_channels + 1, 4, 4, 4),
                        "tex_encoder.bias": (tex_feat_channels,)})
        self._decode_names = list(shapes)
        gen = torch.Generator().manual_seed(0)
        for name, shape in {**enc, **shapes}.items():
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            if ".norm_" in name:
                t = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
            elif ".out_layers.1." in name:
                t = torch.zeros(shape)                      # zero_module (src/encoding/blocks.py:226-230)
            else:
                t = (torch.rand(shape, generator=gen) * 2 - 1) * (1.0 / max(fan_in, 1)) ** 0.5
            _register(self, name, t)
        self.register_buffer("aabb", torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32))
        self._handle = None
        self._synced = None
        self._prepared_for = None
        self._ae = None              # s3d_ae handle (training tier)
        self._ae_flat = None
        self._ae_layout = None
        self._ae_synced = None
        self._ae_dirty = False
        self._ae_volume = None
        self.tex_group_begin = None
        # the sdftex skip net has its training tier from construction, as it always had; the geometry-only net and the skip net
        # with more than 3 texture channels keep their documented decode-only contract until build_training_tier() is called
        self._tier_built = self.variant == 0 and tex_channels <= 3

    _TEX_VARIANT = 0
    _TEX_PREFIXES = ("tex_encoder", "tex_convs", "tex_decoder")

    def _decode_shapes(self):
        return ae_param_shapes(*self.cfg) if self.use_tex else geo_only_param_shapes(*self.cfg[:1], *self.cfg[2:5])

    @property
    def training_tier_built(self):
        """Whether encode, forward(vol, x), loss_and_grads and flat_parameters run: always for the skip net with up to 3 texture
        channels (sdftex); for the geometry-only net of either class (sdf) and the skip net with up to 8 channels (sdfpbr with
        --enc_net_type skip) once build_training_tier() was called; for the PBR net with texture once
        build_training_tier(material_heads=True) was."""
        return self._tier_built

    def build_training_tier(self, material_heads=False):
        """Switch the s3d_ae_* tier on for this network (ShapeAutoEncoder does before it loads training data).  A network as
        constructed keeps what it did before this tier covered it: the geometry-only and the 8-channel nets decode only and
        say so.  The PBR net with texture trains through s3d_ae_create_pbr and is switched on by naming it:
        build_training_tier(material_heads=True); without the argument it raises NotImplementedError, as it always did."""
        if self.variant not in (0, 1) and not material_heads:
            raise NotImplementedError(
                f"{type(self).__name__}(use_tex={self.use_tex}, tex_channels={self.cfg[5]}): the training tier of the PBR network "
                "with texture is not built by this call: build_training_tier(material_heads=True) switches it on")
        if material_heads and self.variant != 2:
            raise ValueError(f"{type(self).__name__}(use_tex={self.use_tex}): material_heads=True is the PBR network with texture's")
        self._tier_built = True
        return self

    @property
    def loss_names(self):
        """The entries of `loss_and_grads`' losses: the reference's loss_dict keys of this network's data type."""
        if self.variant == 1:
            return ("sdf_loss",)
        return ("sdf_loss", "rgb_loss", "mr_loss", "normal_loss") if self.cfg[5] == 8 else ("sdf_loss", "tex_loss")

    def geo_parameters(self):
        """reference :146-147"""
        return [p for n, p in self.named_parameters() if n.startswith(("geo_encoder", "geo_convs", "geo_decoder"))]

    def tex_parameters(self):
        """reference :149-150 (:260-262 for the PBR net)"""
        return [p for n, p in self.named_parameters() if n.startswith(self._TEX_PREFIXES)]

    def reset_aabb(self, aabb):
        if not isinstance(aabb, torch.Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32)
        self.aabb = aabb.to(self.aabb.device)

    # ------------------------------------------------------------------ training tier (s3d_ae_*)
    def _ensure_ae(self):
        if not self.training_tier_built:
            raise NotImplementedError(
                f"{type(self).__name__}(use_tex={self.use_tex}, tex_channels={self.cfg[5]}): the training tier (encode, "
                "forward(vol, x), loss_and_grads, flat_parameters) of this network is not built yet: call build_training_tier() "
                "first (build_training_tier(material_heads=True) for the PBR network with texture), as ShapeAutoEncoder does "
                "for training")
        lib = _lib.load()
        params = dict(self.named_parameters())
        if self._ae is None:
            h = C.c_void_p()
            cfg = _lib.DecoderCfg(*self.cfg)
            if self.variant == 2:
                _lib.check(lib.s3d_ae_create_pbr(C.byref(cfg), C.byref(h)))
            else:
                _lib.check(lib.s3d_ae_create_variant(C.byref(cfg), self.variant, C.byref(h)))
            assert lib.s3d_ae_out_channels(h) == self.out_channels
            self._ae = h
        intact = self._ae_flat is not None and all(
            params[n].data_ptr() == self._ae_flat.data_ptr() + 4 * off and params[n].device == self._ae_flat.device
            for n, off, _, _ in self._ae_layout)
        if not intact:
            dev = next(iter(params.values())).device
            _lib.require_gpu(next(iter(params.values())))
            layout = _lib.read_layout(lib.s3d_ae_num_params(self._ae),
                                      lambda i, *refs: _lib.check(lib.s3d_ae_param_info(self._ae, i, *refs)))
            tb = C.c_int64()
            total = lib.s3d_ae_param_numel(self._ae, C.byref(tb))
            flat = torch.empty(total, device=dev, dtype=torch.float32)
            with torch.no_grad():
                for name, off, numel, shp in layout:
                    p = params[name]
                    assert tuple(p.shape) == shp, (name, tuple(p.shape), shp)
                    view = flat[off:off + numel].view(shp)
                    view.copy_(p.detach().to(dev, torch.float32))
                    p.data = view
            with torch.cuda.device(dev):
                _lib.check(lib.s3d_ae_attach(self._ae, _lib.ptr(flat), total))
            self._ae_flat, self._ae_layout, self.tex_group_begin = flat, layout, int(tb.value)
            self._ae_synced = None
            self._ae_volume = None
            params = dict(self.named_parameters())
        stamp = tuple((p.data_ptr(), p._version) for p in params.values())
        if stamp != self._ae_synced or self._ae_dirty:
            with torch.cuda.device(self._ae_flat.device):
                _lib.check(lib.s3d_ae_repack(self._ae, _lib.stream_ptr()))
            self._ae_synced, self._ae_dirty = stamp, False
        return lib

    @property
    def flat_parameters(self):
        self._ensure_ae()
        return self._ae_flat

    def mark_parameters_changed(self):
        """After writing to flat_parameters directly (fused optimizer): repack before the next use."""
        self._ae_dirty = True
        self._synced = None            # the decode handle mirrors the parameters from the host side
        self._prepared_for = None

    def split_flat(self, flat):
        self._ensure_ae()
        return {name: flat[off:off + numel].view(shp) for name, off, numel, shp in self._ae_layout}

    def set_volume(self, vol):
        """vol [1, out_channels, 2H, 2W, 2D] (sdf, then the texture channels): reduce it to the encoder's three projections
        (done once per volume)."""
        lib = self._ensure_ae()
        _lib.require_gpu(vol)
        v = vol.contiguous().float()
        assert v.dim() == 5 and v.shape[0] == 1, tuple(v.shape)
        key = (v.data_ptr(), v._version, tuple(v.shape))
        if key != self._ae_volume:
            with torch.cuda.device(v.device):
                _lib.check(lib.s3d_ae_set_volume(self._ae, _lib.ptr(v), v.shape[1], v.shape[2], v.shape[3], v.shape[4],
                                                 _lib.stream_ptr()))
                torch.cuda.current_stream().synchronize()      # the library keeps projections, not `v`
            self._ae_volume = key
            self._feat_size = (v.shape[2] // 2, v.shape[3] // 2, v.shape[4] // 2)
        return lib

    def encode(self, vol):
        """reference :164-180 -> [xy [1,C,H,W], xz [1,C,H,D], yz [1,C,W,D]]"""
        lib = self.set_volume(vol)
        H, W, D = self._feat_size
        Cc = self.in_feat_channels
        dev = vol.device
        out = [torch.empty((1, Cc, a, b), device=dev, dtype=torch.float32) for a, b in ((H, W), (H, D), (W, D))]
        with torch.cuda.device(dev):
            _lib.check(lib.s3d_ae_encode(self._ae, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()))
        return out

    def loss_and_grads(self, vol, pts, sdf, tex, loss_cfg, aabb=None, grad_out=None, want_pred=False):
        """One ShapeAutoEncoder iteration without the optimizer (model.py:186-237 + loss.backward()): returns
        (losses on the device, pred or None, flat gradient of their sum).  losses is [2] = (sdf_loss, tex_loss) for sdftex and
        for sdf (tex=None, tex_loss 0), and [4] = (sdf_loss, rgb_loss, mr_loss, normal_loss) for the 8 channels of sdfpbr."""
        lib = self.set_volume(vol)
        pts, sdf = pts.contiguous().float(), sdf.contiguous().float()
        N = pts.shape[0]
        dev = pts.device
        if self.variant == 1:
            tex = None
        else:
            tex = tex.contiguous().float()
            assert tuple(tex.shape) == (N, self.cfg[5]), (tuple(tex.shape), N, self.cfg[5])
        assert sdf.numel() == N, (tuple(sdf.shape), N)
        groups = len(self.loss_names) == 4
        losses = torch.empty(4 if groups else 2, device=dev, dtype=torch.float32)
        pred = torch.empty((N, self.out_channels), device=dev, dtype=torch.float32) if want_pred else None
        g = grad_out if grad_out is not None else torch.empty_like(self._ae_flat)
        fn = lib.s3d_ae_loss_grads_groups if groups else lib.s3d_ae_loss_grads
        with torch.cuda.device(dev):
            _lib.check(fn(self._ae, _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(tex), N, self._aabb6(aabb),
                          C.byref(loss_cfg), _lib.ptr(losses), _lib.ptr(pred), _lib.ptr(g), _lib.stream_ptr()))
        return losses, pred, g

    # ------------------------------------------------------------------ HIP handle
    def _ensure_handle(self):
        lib = _lib.load()
        if self._handle is None:
            h = C.c_void_p()
            cfg = _lib.DecoderCfg(*self.cfg)
            _lib.check(lib.s3d_decoder_create_variant(C.byref(cfg), self.variant, C.byref(h)))
            assert lib.s3d_decoder_out_channels(h) == self.out_channels
            self._handle = h
        params = dict(self.named_parameters())
        stamp = tuple((params[n].data_ptr(), params[n]._version) for n in self._decode_names)
        if stamp != self._synced:
            for name in self._decode_names:
                host = params[name].detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * host.dim())(*host.shape)
                _lib.check(lib.s3d_decoder_set_param(self._handle, name.encode(), C.c_void_p(host.data_ptr()), shape,
                                                     host.dim()))
            self._synced = stamp
            self._prepared_for = None
        return lib

    def __del__(self):
        h = self.__dict__.pop("_handle", None)      # not via nn.Module.__setattr__: it may run at interpreter exit
        a = self.__dict__.pop("_ae", None)
        try:
            if h is not None:
                _lib.load().s3d_decoder_destroy(h)
            if a is not None:
                _lib.load().s3d_ae_destroy(a)
        except Exception:
            pass

    def prepare(self, feat_maps):
        """Run geo_convs / tex_convs for this triplane (cached by tensor identity and version)."""
        lib = self._ensure_handle()
        fm = [f.contiguous().float() for f in feat_maps]
        for f in fm:
            _lib.require_gpu(f)
            assert f.dim() == 4 and f.shape[0] == 1 and f.shape[1] == self.in_feat_channels, (tuple(f.shape), self.in_feat_channels)
        key = tuple((f.data_ptr(), f._version, tuple(f.shape)) for f in feat_maps)
        if key == self._prepared_for:
            return lib
        H, W = fm[0].shape[-2:]
        D = fm[1].shape[-1]
        assert fm[1].shape[-2] == H and tuple(fm[2].shape[-2:]) == (W, D)
        with torch.cuda.device(fm[0].device):
            _lib.check(lib.s3d_decoder_prepare_triplane(self._handle, _lib.ptr(fm[0]), _lib.ptr(fm[1]), _lib.ptr(fm[2]),
                                                        H, W, D, _lib.stream_ptr()))
        self._prepared_for = key
        self._keepalive = fm
        return lib

    def _aabb6(self, aabb):
        a = self.aabb if aabb is None else aabb
        a = a.detach().to("cpu", torch.float32).reshape(6)
        return (C.c_float * 6)(*[float(v) for v in a])

    def decode(self, x, feat_maps, aabb=None, clamp_color=False):
        """x [N,3] -> [N, out_channels]: (sdf, sigmoid(tex)) for the skip net (reference :192-220), (sdf) without texture,
        (sdf, rgb, metallic, roughness, normal) unactivated for the PBR net (:293-316).  clamp_color clamps columns >= 1."""
        lib = self.prepare(feat_maps)
        _lib.require_gpu(x)
        pts = x.contiguous().float()
        out = torch.empty((pts.shape[0], self.out_channels), device=pts.device, dtype=torch.float32)
        with torch.cuda.device(pts.device):
            _lib.check(lib.s3d_decoder_decode_points(self._handle, _lib.ptr(pts), pts.shape[0], self._aabb6(aabb),
                                                     int(bool(clamp_color)), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def _sdf_grad(self, x, feat_maps, aabb, iters, max_step, max_move):
        lib = self.prepare(feat_maps)
        _lib.require_gpu(x)
        pts = x.contiguous().float()
        n, dev = pts.shape[0], pts.device
        sdf = torch.empty((n,), device=dev, dtype=torch.float32)
        grad = torch.empty((n, 3), device=dev, dtype=torch.float32)
        moved = torch.empty((n, 3), device=dev, dtype=torch.float32) if iters > 0 else None
        with torch.cuda.device(dev):
            _lib.check(lib.s3d_decoder_sdf_grad(self._handle, _lib.ptr(pts), n, self._aabb6(aabb), int(iters), float(max_step),
                                                float(max_move), _lib.ptr(moved), _lib.ptr(sdf), _lib.ptr(grad), _lib.stream_ptr()))
        return moved, sdf, grad

    def sdf_and_grad(self, x, feat_maps, aabb=None):
        """x [N,3] -> (sdf [N], d sdf / d x [N,3] in world units): the geometry head and its exact gradient with respect to the
        point, with F.grid_sample's autograd conventions (0 beyond a plane's border, the floor cell at a texel centre).  sdf has
        the bits of decode(...)[:, 0]."""
        _, sdf, grad = self._sdf_grad(x, feat_maps, aabb, 0, 0.0, 0.0)
        return sdf, grad

    def project_to_surface(self, x, feat_maps, aabb=None, iters=2, max_step=0.05, max_move=0.1):
        """`iters` Newton steps of x onto the zero level set, x <- x - clamp(sdf g / |g|^2, +-max_step) per component, the
        displacement from the start clamped to +-max_move per component (world units) -> (x', sdf(x'), grad(x'))."""
        if iters == 0:
            sdf, grad = self.sdf_and_grad(x, feat_maps, aabb)
            return x.contiguous().float().clone(), sdf, grad
        return self._sdf_grad(x, feat_maps, aabb, iters, max_step, max_move)

    def decode_grid(self, feat_maps, reso, aabb=None):
        """Cell-centred grid over aabb, colours clamped to [0,1] (decode_grid + decode_batch, model.py:319-349)."""
        lib = self.prepare(feat_maps)
        a6 = self._aabb6(aabb)
        dims = (C.c_int * 3)()
        _lib.check(lib.s3d_decoder_grid_dims(a6, int(reso), dims))
        dev = feat_maps[0].device
        out = torch.empty((dims[0], dims[1], dims[2], self.out_channels), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.s3d_decoder_decode_grid(self._handle, int(reso), a6, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def plane_features(self, feat_maps, group):
        """The prepared feature maps of one group as the reference's [1, up, h, w] tensors: "geo" = geo_convs(...), "tex" =
        tex_convs(...), "tex0" = the PBR net's texture planes after tex_convs[0]."""
        lib = self.prepare(feat_maps)
        gi = {"geo": 0, "tex": 1, "tex0": 2}[group]
        H, W = feat_maps[0].shape[-2:]
        D = feat_maps[1].shape[-1]
        dev = feat_maps[0].device
        outs = [torch.empty((1, self.cfg[2], a, b), device=dev, dtype=torch.float32) for a, b in ((H, W), (H, D), (W, D))]
        with torch.cuda.device(dev):
            for p, o in enumerate(outs):
                _lib.check(lib.s3d_decoder_plane_features(self._handle, gi, p, _lib.ptr(o), _lib.stream_ptr()))
        return outs

    def forward(self, vol, x, aabb=None):
        """net(vol, x) (reference :222-224) through the training-tier forward (no gradient)."""
        lib = self.set_volume(vol)
        pts = x.contiguous().float()
        pred = torch.empty((pts.shape[0], self.out_channels), device=pts.device, dtype=torch.float32)
        with torch.cuda.device(pts.device):
            _lib.check(lib.s3d_ae_forward(self._ae, _lib.ptr(pts), pts.shape[0], self._aabb6(aabb), _lib.ptr(pred), _lib.stream_ptr()))
        return pred


class AutoEncoderGroupPBR(AutoEncoderGroupSkip):
    """Reference :227-316: the geo side of the skip net; tex_convs = two 3x3 blocks (the second normalises its input and adds
    that normalised input back); rgb / mr / normal heads on one gathered feature, no sigmoid.  With texture it trains through
    s3d_ae_create_pbr once build_training_tier(material_heads=True) was called (the tex group is the encoder, both blocks and
    the three heads, :260-262); with use_tex=False it is the base class's geometry-only net and trains like it.  The handle, the
    triplane cache, `decode`, `decode_grid`, `prepare`, `reset_aabb` and the parameter groups are the base class's."""
    _TEX_VARIANT = 2
    _TEX_PREFIXES = ("tex_encoder", "tex_convs", "rgb_decoder", "mr_decoder", "normal_decoder")

    def _decode_shapes(self):
        return pbr_param_shapes(*self.cfg, use_tex=self.use_tex)
