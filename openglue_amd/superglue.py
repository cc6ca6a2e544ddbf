"""Drop-in `SuperGlue` module for OpenGlue's scaffolding, backed by the gfx950 HIP library.

Mirrors the reference plugin point (models/superglue/superglue.py:11-72):
    SuperGlue(config)            same config keys (SURVEY.md §5 "Config")
    .forward(data) -> {'context_descriptors0', 'context_descriptors1', 'scores'}
    .state_dict() / .load_state_dict()   same names and shapes, so Lightning
                                         checkpoints of the reference load unchanged
and adds `.match(data, match_threshold)` = forward + the mutual-NN extraction that
MatchingTrainingModule.forward / OpenGlueMatcher.forward run on `scores`
(models/matching_module.py:174-187, inference.py:176-190).

The torch.nn modules below are PARAMETER CONTAINERS only (they give identical names, shapes and
default initialisation); none of their forward() methods is ever called.  All arithmetic is in
libopenglue_amd.so, reached through the C ABI of include/openglue_amd.h.  There is no CPU or
eager-PyTorch fallback: off-GPU inputs or a missing library raise.  eval(): the fused inference path (og_forward);
train(): openglue_amd.train (the same forward in training mode under autograd, HIP forward/backward kernels).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib

_ENCODERS = ("FeedForwardNet", "FeedForwardNetSiren")
_ATTENTIONS = ("softmax", "linear", "favor_relu")      # 'favor_softmax' is unreachable upstream (NameError, models/superglue/__init__.py:26)


def _mlp_container(*sizes: int) -> nn.Sequential:
    """Same child indices as the reference FeedForwardNet (models/utils.py:48-58):
    conv 3i, relu 3i+1, bn 3i+2, ..., last conv."""
    layers: List[nn.Module] = []
    for i in range(1, len(sizes) - 1):
        layers += [nn.Conv1d(sizes[i - 1], sizes[i], kernel_size=1), nn.ReLU(inplace=True), nn.BatchNorm1d(sizes[i])]
    layers.append(nn.Conv1d(sizes[-2], sizes[-1], kernel_size=1))
    return nn.Sequential(*layers)


def _siren_container(*sizes: int) -> nn.Sequential:
    """Same child indices as the reference FeedForwardNetSiren (models/utils.py:32-45): conv 2i, Sine 2i+1, last conv.
    (The reference's special sine_init only matters for training from scratch; weights are loaded here.)"""
    layers: List[nn.Module] = []
    for i in range(1, len(sizes) - 1):
        layers += [nn.Conv1d(sizes[i - 1], sizes[i], kernel_size=1), nn.Identity()]
    layers.append(nn.Conv1d(sizes[-2], sizes[-1], kernel_size=1))
    return nn.Sequential(*layers)


class _FavorFeatures(nn.Module):
    """Buffer container named like the reference's GeneralizedFavorAttention (attention.py:43-95; created by
    get_attention_mechanism(embed_dim, 'favor_relu'), __init__.py:19-25, as `mha.attention_func`): `projection_matrix`
    [2 * embed_dim, embed_dim], drawn like FavorAttention.sample_orthogonal_random_vectors, and `resample_projection()` for the
    redraw callback (utils/lightning_callbacks.py:6-14).  Its `forward` is never called -- the arithmetic runs in the HIP kernels on
    the packed projection."""

    def __init__(self, embed_dim: int):
        super().__init__()
        from .synthetic import orthogonal_random_features
        self.embed_dim, self.num_orthogonal_features = embed_dim, 2 * embed_dim
        self.register_buffer("projection_matrix", orthogonal_random_features(self.num_orthogonal_features, embed_dim))

    @torch.no_grad()
    def resample_projection(self) -> None:
        from .synthetic import orthogonal_random_features
        new = orthogonal_random_features(self.num_orthogonal_features, self.embed_dim)
        self.projection_matrix.copy_(new.to(self.projection_matrix.device))      # in place: bumps _version, the packed weights re-pack


# The reference's redraw callback (utils/lightning_callbacks.py:6-14) finds the modules to redraw with `isinstance(module, FavorAttention)`,
# FavorAttention being the HOST application's class (models/superglue/attention.py:43).  A host that wants that callback to work UNMODIFIED
# registers its class once -- `openglue_amd.superglue.register_favor_base(FavorAttention)` -- or passes it per model
# (`SuperGlue(config, favor_base=FavorAttention)`); the buffer containers then derive from it and use ITS sampler.  Explicit opt-in: nothing
# is imported from the host's tree behind its back, and without a registration the container is the plain nn.Module above (the branch
# the GPU box tests).  [Round 4 sniffed `models.superglue.attention` off sys.path at import time: class hierarchy and sampler depended on
# the import order of the process.]
_FAVOR_BASE: Optional[type] = None
_HOSTED_FAVOR: dict = {}


def register_favor_base(cls: Optional[type]) -> None:
    """Make the FAVOR buffer containers of every SuperGlue constructed from now on instances of `cls` (the host's FavorAttention:
    `cls(embed_dim, num_orthogonal_features=...)` must register a `projection_matrix` buffer and offer `resample_projection()`);
    None restores the built-in container."""
    global _FAVOR_BASE
    if cls is not None and not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError("register_favor_base: expected an nn.Module subclass (the host's models.superglue.attention.FavorAttention) or None")
    _FAVOR_BASE = cls


_FAVOR_WARNED = False


def _favor_container(embed_dim: int, base: Optional[type]) -> nn.Module:
    if base is None:
        # a host that HAS the reference's FavorAttention loaded but did not register it gets no redraws from the reference's
        # FavorAttentionProjectionRedrawCallback (its isinstance test matches nothing) -- say so once; nothing is imported from the host.
        global _FAVOR_WARNED
        import sys
        if not _FAVOR_WARNED and "models.superglue.attention" in sys.modules:
            _FAVOR_WARNED = True
            import warnings
            warnings.warn("openglue_amd: attention = 'favor_relu' without a registered FavorAttention base: the host's "
                          "FavorAttentionProjectionRedrawCallback (isinstance(module, FavorAttention)) will not find these modules and the "
                          "projection is never resampled.  Call openglue_amd.superglue.register_favor_base(models.superglue.attention."
                          "FavorAttention) or pass SuperGlue(config, favor_base=...) -- INTEGRATION.md.", RuntimeWarning, stacklevel=3)
        return _FavorFeatures(embed_dim)
    cls = _HOSTED_FAVOR.get(base)
    if cls is None:
        # the host's own constructor registers `projection_matrix` with the host's sampler; its resample_projection() copies in place
        cls = type("_HostedFavorFeatures", (base,), {"__doc__": "FAVOR buffer container derived from the registered host class; forward is never called."})
        _HOSTED_FAVOR[base] = cls
    mod = cls(embed_dim, num_orthogonal_features=2 * embed_dim)
    pm = getattr(mod, "projection_matrix", None)
    if not torch.is_tensor(pm) or tuple(pm.shape) != (2 * embed_dim, embed_dim) or not callable(getattr(mod, "resample_projection", None)):
        raise TypeError(f"favor base {base.__name__}: expected a projection_matrix buffer [{2 * embed_dim}, {embed_dim}] and resample_projection()")
    return mod


class _Holder(nn.Module):
    """A named bag of sub-modules (keeps the reference's attribute paths)."""

    def __init__(self, **children: nn.Module):
        super().__init__()
        for k, v in children.items():
            self.add_module(k, v)


def _get_wh(data: Mapping, idx: int):
    """superglue.py:35-38."""
    if "image0" in data and "image1" in data:
        h, w = data[f"image{idx}"].shape[-2:]
        return float(w), float(h)
    w, h = data[f"image{idx}_size"][:2]
    return float(w), float(h)


class _EvalFastPathOutputs(torch.autograd.Function):
    """Marks the outputs of the fused eval-mode path as produced from the parameters WITHOUT a backward: asking for a gradient
    through them raises instead of silently treating them as constants."""

    @staticmethod
    def forward(ctx, anchor, *outs):
        return tuple(o.view_as(o) for o in outs)

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("openglue_amd.SuperGlue: the fused eval-mode path (og_forward) is not differentiable.  Set "
                           "model.eval_autograd = True (eval-mode forward through the autograd kernels, BatchNorm on running "
                           "statistics), call model.train(), or run inference under torch.no_grad().")


class SuperGlue(nn.Module):
    def __init__(self, config: Mapping, favor_base: Optional[type] = None):
        super().__init__()
        self.config = config
        favor_base = favor_base if favor_base is not None else _FAVOR_BASE       # explicit: register_favor_base() / this argument
        pe = dict(config["positional_encoding"])
        gnn = dict(config["attention_gnn"])
        enc_name = pe.get("encoder_name", "FeedForwardNet")
        if enc_name not in _ENCODERS:      # reference: NameError from get_positional_encoder (__init__.py:39-42)
            raise NameError(f"{enc_name} module was not found among positional encoders supported on MI355X: {_ENCODERS}")
        attn = gnn.get("attention", "softmax")
        if attn not in _ATTENTIONS:
            raise ValueError(f"Attention type {attn} is not supported by the MI355X path (supported: {_ATTENTIONS}).")
        D = int(config["descriptor_dim"])
        if int(gnn["embed_dim"]) != D or int(pe["output_size"]) != D:
            raise ValueError("descriptor_dim, attention_gnn.embed_dim and positional_encoding.output_size must agree")
        self.descriptor_dim = D
        self.hidden = [int(h) for h in (pe.get("hidden_layers_sizes") or [])]
        self.side_info_size = int(pe.get("side_info_size", 1))
        self.num_stages, self.num_heads = int(gnn["num_stages"]), int(gnn["num_heads"])
        self.use_offset = bool(gnn.get("use_offset", False))
        self.linear_attention = attn == "linear"
        self.favor_relu = attn == "favor_relu"
        if self.favor_relu and (self.num_heads != 1 or D > 256):
            # the reference multiplies its [2D, D] feature buffer with per-head [B, H, D/H, N] tensors (attention.py:94): with more
            # than one head torch.matmul raises inside forward; fail at construction instead
            raise ValueError("attention 'favor_relu' runs with num_heads == 1 only (as in the reference) and descriptor_dim <= 256")
        self.residual = bool(config.get("residual", False))
        self.no_descriptors = bool(config.get("no_descriptors", False))
        # eval() with autograd enabled and something requiring a gradient: False (default) = the fused inference kernels, outputs
        # attached to a node that raises on backward; True = the differentiable eval-mode path (openglue_amd.train, frozen BatchNorm)
        self.eval_autograd = False

        # ---- parameter tree with the reference's names ----
        self.siren = enc_name == "FeedForwardNetSiren"
        make_enc = _siren_container if self.siren else _mlp_container
        self.positional_encoding = _Holder(encoder=make_enc(2 + self.side_info_size, *self.hidden, D))
        layers = nn.ModuleList()
        for _ in range(2 * self.num_stages):       # even = self, odd = cross (attention_gnn.py:84-89)
            favor = dict(attention_func=_favor_container(D, favor_base)) if self.favor_relu else {}
            mha = _Holder(**favor, in_proj_q=nn.Conv1d(D, D, 1), in_proj_k=nn.Conv1d(D, D, 1),
                          in_proj_v=nn.Conv1d(D, D, 1), out_proj=nn.Conv1d(D, D, 1))
            layers.append(_Holder(module=_Holder(mha=mha, fc=_mlp_container(2 * D, 2 * D, D))))
        self.attention_gnn = _Holder(layers=layers)
        if self.residual:
            self.mix_coefs = nn.Parameter(torch.zeros(D, 1))
        self.linear_proj = nn.Conv1d(D, D, kernel_size=1)
        self.dustbin_score = nn.Parameter(torch.tensor(float(config["dustbin_score_init"])))

        weights_path = config.get("weights", None)
        if weights_path is not None:                 # superglue.py:25-27
            print("SuperGlue loading... ", self.load_state_dict(torch.load(str(weights_path), map_location="cpu")))

        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._tensor_cache = None
        self._workspace: Dict[str, tuple] = {}

    # ------------------------------------------------------------------ shape / packing
    def _shape(self, B: int, m: int, n: int, match_threshold: float = 0.0) -> _lib.og_shape:
        s = _lib.og_shape()
        s.batch, s.m, s.n = B, m, n
        s.desc_dim, s.num_heads, s.num_stages = self.descriptor_dim, self.num_heads, self.num_stages
        s.side_info, s.num_hidden = self.side_info_size, len(self.hidden)
        for i, h in enumerate(self.hidden):
            s.hidden[i] = h
        s.sinkhorn_iters = int(self.config["otp"]["num_iters"])
        s.sinkhorn_reg = float(self.config["otp"]["reg"])
        s.flags = ((_lib.OG_FLAG_RESIDUAL if self.residual else 0) | (_lib.OG_FLAG_USE_OFFSET if self.use_offset else 0)
                   | (_lib.OG_FLAG_NO_DESCRIPTORS if self.no_descriptors else 0)
                   | (_lib.OG_FLAG_SIREN_ENCODER if self.siren else 0)
                   | (_lib.OG_FLAG_LINEAR_ATTENTION if self.linear_attention else 0)
                   | (_lib.OG_FLAG_FAVOR_RELU if self.favor_relu else 0))
        s.match_threshold = float(match_threshold)
        return s

    def _tensors(self):
        """Parameters and buffers, cached: walking the module tree (~250 tensors) on every call costs more than the
        launch sequence of a single small pair.  Invalidated by _apply (.to/.cuda/.float) and load_state_dict; a caller
        that REPLACES Parameter objects by hand calls invalidate_packed()."""
        if self._tensor_cache is None:
            self._tensor_cache = list(self.parameters()) + list(self.buffers())
        return self._tensor_cache

    def invalidate_packed(self) -> None:
        self._tensor_cache = None
        self._packed = None
        self._packed_key = None

    def _apply(self, fn, *a, **kw):
        self.invalidate_packed()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.invalidate_packed()
        return super().load_state_dict(*a, **kw)

    def _param_key(self, device):
        ts = self._tensors()
        # in-place updates (optimizer steps, copy_) bump _version; storage swaps (p.data = w, swap_tensors, set_) change data_ptr;
        # moves re-create the tensors (_apply above).  Inference-mode tensors have no version counter.
        def ver(t):
            try:
                return t._version
            except RuntimeError:
                return -1
        return (str(device),) + tuple((t.data_ptr(), ver(t)) for t in ts)

    def check_status(self) -> int:
        """Synchronise and report how the optimal-transport stage of the LAST forward / match call went (og_forward_status): 0 = normal;
        2 = its on-chip-resident kernel (large co-resident batches) timed out waiting for a peer workgroup and the safety-net kernel
        behind it recomputed the solve (scores valid, call slow) -- a RuntimeWarning; anything else raises RuntimeError.  A no-op
        (0) before the first call."""
        last = getattr(self, "_last_call", None)
        if last is None:
            return 0
        shape, ws, stream = last
        with torch.cuda.device(ws.device):
            stream.synchronize()      # the stream the call was ENQUEUED on (not whatever is current now): og_forward_status itself only waits for the NULL stream
            rc = _lib.load().og_forward_status(C.byref(shape), ws.data_ptr())
        if rc == 2:
            import warnings
            warnings.warn("og_forward_status = 2: the resident Sinkhorn kernel timed out (CUs held by another stream / process?); "
                          "the fallback kernel recomputed the scores", RuntimeWarning)
        elif rc == 3:
            raise RuntimeError("og_forward_status = 3: non-finite scores -- an activation left the binary16 range of the split-f16 "
                               "operands (|x| >= 65504) or the inputs / weights hold NaN or Inf")
        elif rc != 0:
            raise RuntimeError(f"og_forward_status = {rc}: the last call's Sinkhorn stage did not complete (scores invalid)")
        return rc

    def _get_workspace(self, dev, key, nbytes: int) -> torch.Tensor:
        """One live workspace per device, keyed by CAPACITY: any call whose og_workspace_bytes fits re-uses it, whatever its (B, m, n) -- real
        pairs (inference.py) have a different keypoint count on every call.  It only grows (by at least a quarter, so a slowly rising count
        does not re-allocate per call); og_forward re-arms everything it keeps in there (counters, status, exchange granules) on every call,
        so no state of an earlier shape is ever read.  `key` is informational (kept for debugging: the shape that last sized it)."""
        wkey = str(dev)
        ent = self._workspace.get(wkey)
        if ent is None or ent[0].numel() < nbytes:
            grow = 0 if ent is None else ent[0].numel() + ent[0].numel() // 4
            self._workspace.pop(wkey, None)      # drop the old buffer before the new one is requested
            ent = None
            ws = torch.empty(max(nbytes, grow), device=dev, dtype=torch.uint8)
            ent = (ws, tuple(key))
            self._workspace[wkey] = ent
        return ent[0]

    def _pack(self, device: torch.device) -> torch.Tensor:
        """Packed weights on `device`, cached until a parameter changes."""
        key = self._param_key(device)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        self._packed = torch.from_numpy(self.pack_host()).to(device)
        self._packed_key = key
        return self._packed

    def pack_host(self) -> np.ndarray:
        """og_pack_weights on host copies of the parameters -> float32 blob (layout: og_packed_layout)."""
        lib = _lib.load()
        shape = self._shape(1, 1, 1)
        keep: List[np.ndarray] = []

        def host(t: torch.Tensor) -> int:
            a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            keep.append(a)
            return a.ctypes.data

        def conv(mod: nn.Conv1d) -> _lib.og_conv:
            return _lib.og_conv(host(mod.weight), host(mod.bias))

        def bn(mod: nn.BatchNorm1d) -> _lib.og_bn:
            return _lib.og_bn(host(mod.weight), host(mod.bias), host(mod.running_mean), host(mod.running_var))

        P = _lib.og_params()
        enc = self.positional_encoding.encoder
        for i in range(len(self.hidden) + 1):
            if self.siren:
                P.enc_conv[i] = conv(enc[2 * i])
            else:
                P.enc_conv[i] = conv(enc[3 * i])
                if i < len(self.hidden):
                    P.enc_bn[i] = bn(enc[3 * i + 2])
        LayerArr = _lib.og_layer_params * max(1, 2 * self.num_stages)
        layer_arr = LayerArr()
        for l, holder in enumerate(self.attention_gnn.layers):
            mod = holder.module
            lp = layer_arr[l]
            lp.in_proj_q, lp.in_proj_k = conv(mod.mha.in_proj_q), conv(mod.mha.in_proj_k)
            lp.in_proj_v, lp.out_proj = conv(mod.mha.in_proj_v), conv(mod.mha.out_proj)
            lp.fc0, lp.fc_bn, lp.fc3 = conv(mod.fc[0]), bn(mod.fc[2]), conv(mod.fc[3])
            lp.favor_projection = host(mod.mha.attention_func.projection_matrix) if self.favor_relu else None
        P.layers = C.cast(layer_arr, C.POINTER(_lib.og_layer_params))
        P.linear_proj = conv(self.linear_proj)
        P.mix_coefs = host(self.mix_coefs) if self.residual else None
        P.dustbin_score = float(self.dustbin_score.detach())
        nbytes = lib.og_packed_weights_bytes(C.byref(shape))
        if nbytes == 0:
            _lib.check(lib.og_check_shape(C.byref(shape)), "og_check_shape")
        blob = np.empty(nbytes // 4, dtype=np.float32)
        _lib.check(lib.og_pack_weights(C.byref(shape), C.byref(P), blob.ctypes.data), "og_pack_weights")
        return blob

    # ------------------------------------------------------------------ the hot path
    def _run(self, data: Mapping, want_matches: bool, match_threshold: float, both_sides: bool, _profile=None, _tap=None) -> Dict[str, torch.Tensor]:
        if self.training:
            raise RuntimeError("match() / the fused og_forward path run in eval() mode only (BatchNorm on running statistics); the "
                               "training-mode forward is SuperGlue.forward in train() (openglue_amd.train)")
        lib = _lib.load()
        names = ("keypoints0", "keypoints1", "local_descriptors0", "local_descriptors1", "side_info0", "side_info1")
        t = {}
        for k in names:
            v = data[k]
            if not isinstance(v, torch.Tensor) or not v.is_cuda:
                raise RuntimeError(f"data['{k}'] must be a tensor on the MI355X; openglue_amd has no CPU fallback")
            t[k] = v.detach().to(torch.float32).contiguous()
        dev = t["keypoints0"].device
        if t["keypoints0"].dim() != 3 or t["keypoints1"].dim() != 3:
            raise ValueError("keypoints must be [B, n, 2]")
        B, m, _ = t["keypoints0"].shape
        n = t["keypoints1"].shape[1]
        D, s = self.descriptor_dim, self.side_info_size
        if t["keypoints0"].shape != (B, m, 2) or t["keypoints1"].shape != (B, n, 2):
            raise ValueError("keypoints0 / keypoints1 must be [B, m, 2] / [B, n, 2] with the same batch size")
        if any(v.device != dev for v in t.values()):
            raise ValueError("all input tensors must be on the same device")
        if t["local_descriptors0"].shape != (B, m, D) or t["local_descriptors1"].shape != (B, n, D):
            raise ValueError("local_descriptors must be [B, n, descriptor_dim]")
        if t["side_info0"].shape != (B, m, s) or t["side_info1"].shape != (B, n, s):
            raise ValueError("side_info must be [B, n, side_info_size]")
        shape = self._shape(B, m, n, match_threshold)
        _lib.check(lib.og_check_shape(C.byref(shape)), "og_check_shape")
        with torch.cuda.device(dev):
            packed = self._pack(dev)
            ws = self._get_workspace(dev, (B, m, n), lib.og_workspace_bytes(C.byref(shape)))
            self._last_call = (shape, ws, torch.cuda.current_stream(dev))      # check_status() drains THIS stream
            out = {
                "context_descriptors0": torch.empty(B, D, m, device=dev, dtype=torch.float32),
                "context_descriptors1": torch.empty(B, D, n, device=dev, dtype=torch.float32),
                "scores": torch.empty(B, m + 1, n + 1, device=dev, dtype=torch.float32),
            }
            if want_matches:
                out["matches0"] = torch.empty(B, m, device=dev, dtype=torch.int64)
                out["matching_scores0"] = torch.empty(B, m, device=dev, dtype=torch.float32)
                if both_sides:
                    out["matches1"] = torch.empty(B, n, device=dev, dtype=torch.int64)
                    out["matching_scores1"] = torch.empty(B, n, device=dev, dtype=torch.float32)
            inp = _lib.og_inputs(t["keypoints0"].data_ptr(), t["keypoints1"].data_ptr(),
                                 t["local_descriptors0"].data_ptr(), t["local_descriptors1"].data_ptr(),
                                 t["side_info0"].data_ptr() if s else None, t["side_info1"].data_ptr() if s else None)
            inp.image0_wh[0], inp.image0_wh[1] = _get_wh(data, 0)
            inp.image1_wh[0], inp.image1_wh[1] = _get_wh(data, 1)
            ptr = lambda k: out[k].data_ptr() if k in out else None
            o = _lib.og_outputs(ptr("scores"), ptr("context_descriptors0"), ptr("context_descriptors1"),
                                ptr("matches0"), ptr("matching_scores0"), ptr("matches1"), ptr("matching_scores1"))
            if _tap == "encoder":    # the keypoint-encoder stage alone (og_keypoint_encoder): nothing else runs, nothing else is written
                out = {"_tap_x": torch.empty(B * (m + n), D, device=dev, dtype=torch.float32)}
                _lib.call("og_keypoint_encoder", dev, C.byref(shape), C.byref(inp), packed.data_ptr(), ws.data_ptr(), out["_tap_x"].data_ptr(),
                          _lib.STREAM)
                out["_bmn"] = (B, m, n)
                return out
            if _tap is not None:     # per-stage parity tests: the residual stream at one stage boundary (og_forward_tap)
                out["_tap_x"] = torch.empty(B * (m + n), D, device=dev, dtype=torch.float32)
                _lib.call("og_forward_tap", dev, C.byref(shape), C.byref(inp), packed.data_ptr(), ws.data_ptr(), C.byref(o), _lib.STREAM,
                          int(_tap), out["_tap_x"].data_ptr())
            elif _profile is None:
                _lib.call("og_forward", dev, C.byref(shape), C.byref(inp), packed.data_ptr(), ws.data_ptr(), C.byref(o), _lib.STREAM)
            else:      # bench.py: per-kernel-class HIP-event times (synchronises the stream)
                _lib.call("og_forward_profiled", dev, C.byref(shape), C.byref(inp), packed.data_ptr(), ws.data_ptr(), C.byref(o), _lib.STREAM,
                          _profile[0], _profile[1])
        return out

    @torch.no_grad()
    def forward_tap(self, data: Mapping, tap: int):
        """The residual stream at one stage boundary (og_forward_tap): tap 0 = local_descriptors + keypoint encoder as it enters the GNN,
        tap k = after GNN layer k - 1 (reference: attention_gnn.layers[k - 1](desc0, desc1)).  Returns (x0 [B, m, D], x1 [B, n, D])."""
        out = self._run(data, want_matches=False, match_threshold=0.2, both_sides=False, _tap=tap)
        B, _, m = out["context_descriptors0"].shape
        n = out["context_descriptors1"].shape[2]
        x = out["_tap_x"]
        return x[:B * m].view(B, m, -1), x[B * m:].view(B, n, -1)

    @torch.no_grad()
    def encode_keypoints(self, data: Mapping):
        """local_descriptors + keypoint_encoder(normalised keypoints, side info) (superglue.py:44-55, 74-78; positional_encoding.py:16-19)
        through og_keypoint_encoder: only that stage runs.  Returns (x0 [B, m, D], x1 [B, n, D]) -- what enters the attentional GNN."""
        out = self._run(data, want_matches=False, match_threshold=0.2, both_sides=False, _tap="encoder")
        B, m, n = out["_bmn"]
        x = out["_tap_x"]
        return x[:B * m].view(B, m, -1), x[B * m:].view(B, n, -1)

    # ------------------------------------------------------------------ ragged batches (BASELINE config 5)
    _RAGGED_KEYS = ("keypoints0", "keypoints1", "local_descriptors0", "local_descriptors1", "side_info0", "side_info1")

    def pack_ragged(self, pairs) -> Dict[str, object]:
        """Token-pack a list of UN-batched data dicts (keypoints0 [m_i, 2], local_descriptors0 [m_i, D], side_info0
        [m_i, s], ... on the GPU, each with its own image0/image1 tensors or image{0,1}_size = [W, H]) into the layout
        og_forward_ragged consumes: every tensor concatenated over the pairs without padding, plus the host-side
        per-pair lengths and image sizes.  A caller that keeps its features packed can build this dict itself."""
        if not pairs:
            raise ValueError("pack_ragged: empty list of pairs")
        D, s = self.descriptor_dim, self.side_info_size
        dev = None
        for i, p in enumerate(pairs):
            for k in self._RAGGED_KEYS:
                v = p[k]
                if not isinstance(v, torch.Tensor) or not v.is_cuda:
                    raise RuntimeError(f"pairs[{i}]['{k}'] must be a tensor on the MI355X; openglue_amd has no CPU fallback")
                if dev is None:
                    dev = v.device
                if v.device != dev:
                    raise ValueError(f"pairs[{i}]['{k}'] is on {v.device}, expected {dev}")
            for side in (0, 1):
                cnt = p[f"keypoints{side}"].shape[0]
                if tuple(p[f"keypoints{side}"].shape) != (cnt, 2):
                    raise ValueError(f"pairs[{i}]['keypoints{side}'] must be [n, 2]")
                if tuple(p[f"local_descriptors{side}"].shape) != (cnt, D):
                    raise ValueError(f"pairs[{i}]['local_descriptors{side}'] must be [{cnt}, {D}]")
                if tuple(p[f"side_info{side}"].shape) != (cnt, s):
                    raise ValueError(f"pairs[{i}]['side_info{side}'] must be [{cnt}, {s}]")
        out: Dict[str, object] = {k: torch.cat([p[k].detach().to(torch.float32) for p in pairs], 0).contiguous()
                                  for k in self._RAGGED_KEYS}
        out["lens0"] = [int(p["keypoints0"].shape[0]) for p in pairs]
        out["lens1"] = [int(p["keypoints1"].shape[0]) for p in pairs]
        out["image0_wh"] = [_get_wh(p, 0) for p in pairs]         # every pair is normalised with ITS OWN image size
        out["image1_wh"] = [_get_wh(p, 1) for p in pairs]
        return out

    @torch.no_grad()
    def match_ragged_packed(self, packed: Mapping, match_threshold: float = 0.2, both_sides: bool = True,
                            context_descriptors: bool = False, _profile=None) -> List[Dict[str, torch.Tensor]]:
        """One og_forward_ragged call per chunk of 64 pairs on token-packed tensors (see pack_ragged).
        `_profile` (bench.py): a (c_float[OG_NUM_STAGES], c_int32[OG_NUM_STAGES]) pair -> og_forward_ragged_profiled
        (synchronises; per-kernel-class HIP-event times of the LAST chunk)."""
        if self.training:
            raise RuntimeError("openglue_amd.SuperGlue: ragged batches are an inference path; call .eval()")
        lib = _lib.load()
        l0_all, l1_all = list(packed["lens0"]), list(packed["lens1"])
        P = len(l0_all)
        if len(l1_all) != P or len(packed["image0_wh"]) != P or len(packed["image1_wh"]) != P:
            raise ValueError("lens0, lens1, image0_wh, image1_wh must have one entry per pair")
        D, s_ = self.descriptor_dim, self.side_info_size
        t = {k: packed[k] for k in self._RAGGED_KEYS}
        dev = t["keypoints0"].device
        for side, lens in ((0, l0_all), (1, l1_all)):
            tot = sum(lens)
            for k, w in ((f"keypoints{side}", 2), (f"local_descriptors{side}", D), (f"side_info{side}", s_)):
                v = t[k]
                if not isinstance(v, torch.Tensor) or not v.is_cuda or v.device != dev or v.dtype != torch.float32 or not v.is_contiguous():
                    raise RuntimeError(f"packed['{k}'] must be a contiguous fp32 tensor on {dev}")
                if tuple(v.shape) != (tot, w):
                    raise ValueError(f"packed['{k}'] must be [{tot}, {w}], got {tuple(v.shape)}")
        results: List[Dict[str, torch.Tensor]] = []
        r0 = r1 = 0
        for c0 in range(0, P, _lib.OG_MAX_RAGGED):
            l0, l1 = l0_all[c0:c0 + _lib.OG_MAX_RAGGED], l1_all[c0:c0 + _lib.OG_MAX_RAGGED]
            B = len(l0)
            T0, T1 = sum(l0), sum(l1)
            shape = self._shape(B, max(l0), max(l1), match_threshold)
            _lib.check(lib.og_check_shape(C.byref(shape)), "og_check_shape")
            n_scores = sum((a + 1) * (b + 1) for a, b in zip(l0, l1))
            with torch.cuda.device(dev):
                pk = self._pack(dev)
                ws = self._get_workspace(dev, ("ragged", B, max(l0), max(l1)), lib.og_workspace_bytes(C.byref(shape)))
                self._last_call = (shape, ws, torch.cuda.current_stream(dev))     # the ragged path takes the resident Sinkhorn schedule too: check_status() covers it
                scores = torch.empty(n_scores, device=dev, dtype=torch.float32)
                m0 = torch.empty(T0, device=dev, dtype=torch.int64)
                s0 = torch.empty(T0, device=dev, dtype=torch.float32)
                m1 = torch.empty(T1, device=dev, dtype=torch.int64) if both_sides else None
                s1 = torch.empty(T1, device=dev, dtype=torch.float32) if both_sides else None
                c0d = torch.empty(T0 * D, device=dev, dtype=torch.float32) if context_descriptors else None
                c1d = torch.empty(T1 * D, device=dev, dtype=torch.float32) if context_descriptors else None
                sl = lambda k, a, b: t[k][a:b]                       # row slices of contiguous 2-D tensors stay contiguous
                inp = _lib.og_inputs(sl("keypoints0", r0, r0 + T0).data_ptr(), sl("keypoints1", r1, r1 + T1).data_ptr(),
                                     sl("local_descriptors0", r0, r0 + T0).data_ptr(), sl("local_descriptors1", r1, r1 + T1).data_ptr(),
                                     sl("side_info0", r0, r0 + T0).data_ptr() if s_ else None,
                                     sl("side_info1", r1, r1 + T1).data_ptr() if s_ else None)
                wh0 = (C.c_float * (2 * B))(*[v for wh in packed["image0_wh"][c0:c0 + B] for v in wh])
                wh1 = (C.c_float * (2 * B))(*[v for wh in packed["image1_wh"][c0:c0 + B] for v in wh])
                inp.image0_wh[0], inp.image0_wh[1] = wh0[0], wh0[1]
                inp.image1_wh[0], inp.image1_wh[1] = wh1[0], wh1[1]
                o = _lib.og_outputs(scores.data_ptr(), c0d.data_ptr() if context_descriptors else None,
                                    c1d.data_ptr() if context_descriptors else None, m0.data_ptr(), s0.data_ptr(),
                                    m1.data_ptr() if both_sides else None, s1.data_ptr() if both_sides else None)
                a0 = (C.c_int32 * B)(*l0)
                a1 = (C.c_int32 * B)(*l1)
                if _profile is None:
                    _lib.call("og_forward_ragged", dev, C.byref(shape), a0, a1, wh0, wh1, C.byref(inp), pk.data_ptr(), ws.data_ptr(), C.byref(o),
                              _lib.STREAM)
                else:
                    _lib.call("og_forward_ragged_profiled", dev, C.byref(shape), a0, a1, wh0, wh1, C.byref(inp), pk.data_ptr(), ws.data_ptr(),
                              C.byref(o), _lib.STREAM, _profile[0], _profile[1])
            so = o0 = o1 = 0
            for a, b in zip(l0, l1):
                r = {"scores": scores[so:so + (a + 1) * (b + 1)].view(a + 1, b + 1), "matches0": m0[o0:o0 + a],
                     "matching_scores0": s0[o0:o0 + a]}
                if both_sides:
                    r["matches1"], r["matching_scores1"] = m1[o1:o1 + b], s1[o1:o1 + b]
                if context_descriptors:       # channel-first [D, m_i] like the reference (superglue.py:68-72)
                    r["context_descriptors0"] = c0d[o0 * D:(o0 + a) * D].view(D, a)
                    r["context_descriptors1"] = c1d[o1 * D:(o1 + b) * D].view(D, b)
                results.append(r)
                so += (a + 1) * (b + 1); o0 += a; o1 += b
            r0 += T0; r1 += T1
        return results

    @torch.no_grad()
    def match_ragged(self, pairs, match_threshold: float = 0.2, both_sides: bool = True,
                     context_descriptors: bool = False) -> List[Dict[str, torch.Tensor]]:
        """Ragged batch (BASELINE config 5): `pairs[i]` is an UN-batched data dict (keypoints0 [m_i, 2],
        local_descriptors0 [m_i, D], side_info0 [m_i, s], ... on the GPU) with its own image sizes.  All pairs go through
        og_forward_ragged on token-packed tensors (chunks of 64 pairs); the result of every pair equals running it
        alone, which is the only semantics the mask-free reference defines.
        Returns one dict per pair: 'scores' [m_i+1, n_i+1], 'matches0' [m_i], 'matching_scores0' [m_i] (+ side 1,
        + 'context_descriptors{0,1}' [D, m_i] on request)."""
        return self.match_ragged_packed(self.pack_ragged(pairs), match_threshold, both_sides, context_descriptors)

    def forward(self, data: Mapping) -> Dict[str, torch.Tensor]:
        """Same contract as the reference SuperGlue.forward (superglue.py:29-72).  eval(): the fused inference path (og_forward);
        train(): the training path of openglue_amd.train (batch-statistics BatchNorm, autograd through HIP forward/backward kernels)."""
        if self.training:
            from . import train
            return train.superglue_forward_train(self, data)
        wants_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                  or any(torch.is_tensor(v) and v.requires_grad for v in data.values()))
        if wants_grad and self.eval_autograd:
            # eval() under autograd (the reference's forward is differentiable in eval mode: fine-tuning on frozen BatchNorm
            # statistics): the same Functions as the training path, BatchNorm on its running statistics
            from . import train
            return train.superglue_forward_train(self, data, frozen_bn=True)
        with torch.no_grad():
            out = self._run(data, want_matches=False, match_threshold=0.0, both_sides=False)
        if wants_grad:
            # the fused inference kernels have no backward: the outputs stay attached to a node that RAISES when a gradient is
            # asked of it -- never silently detached tensors (set model.eval_autograd = True for the differentiable eval path)
            anchor = next((p for p in self.parameters() if p.requires_grad), None)
            if anchor is None:
                anchor = next(v for v in data.values() if torch.is_tensor(v) and v.requires_grad)
            keys = list(out)
            vals = _EvalFastPathOutputs.apply(anchor, *[out[k] for k in keys])
            out = dict(zip(keys, vals))
        return out

    @torch.no_grad()
    def match(self, data: Mapping, match_threshold: float = 0.2, both_sides: bool = True, _profile=None) -> Dict[str, torch.Tensor]:
        """forward + mutual-NN extraction in one enqueue: adds 'matches0', 'matching_scores0'
        (matching_module.py:183-187) and, with both_sides, 'matches1', 'matching_scores1' (inference.py:183-188)."""
        return self._run(data, want_matches=True, match_threshold=match_threshold, both_sides=both_sides, _profile=_profile)
