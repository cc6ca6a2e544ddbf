"""Seeded synthetic keypoints / descriptors / weights for the SuperGlue hot path.

Used by bench.py, the parity tests and the golden-fixture generator, so that the
same (seed -> tensors) mapping is available on the build box and on the GPU box
without shipping 48 MB of weights.  Everything is generated on the CPU with an
explicit ``torch.Generator`` and is therefore reproducible for a given torch
version (the fixtures under tests/golden/ were produced with the same functions).

Recipe follows SURVEY.md §8(d): keypoints uniform on a 960x720 image, 60 % of the
image-1 keypoints are noisy copies (2 px) of image-0 keypoints with a perturbed copy
of the descriptor, descriptors are unit-norm Gaussians scaled by 32 (the scale stands
in for trained weights: with random-init weights unit-norm descriptors all fall into
the dustbin), side-info U(0,1).  BatchNorm statistics are randomised so that the
Conv -> ReLU -> BN order of the reference (models/utils.py:52-56) is exercised.
"""
from __future__ import annotations

import math
import zlib
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import torch

IMAGE_WH = (960, 720)  # config/config.yaml:10 target_size

# BASELINE.json "configs", as keyword sets understood by make_config().
CONFIGS = {
    "C1": dict(descriptor_dim=64, num_stages=2, num_heads=4, num_iters=3, side_info_size=1,
               kpts=(64, 64), batch=1),
    "C2": dict(descriptor_dim=256, num_stages=9, num_heads=4, num_iters=100, side_info_size=1,
               kpts=(1024, 1024), batch=32),
    "C3": dict(descriptor_dim=256, num_stages=9, num_heads=4, num_iters=100, side_info_size=1,
               kpts=(2048, 2048), batch=32),   # 256 pairs over 8 GPUs -> 32 per GPU
    "C4": dict(descriptor_dim=128, num_stages=9, num_heads=4, num_iters=100, side_info_size=6,
               kpts=(4096, 4096), batch=8),    # 64 pairs over 8 GPUs -> 8 per GPU
    # not a BASELINE config: the reference's OWN shipped operating point for its 128-d feature family -- config/features/sift_opencv.yaml:2-4
    # (descriptor_dim 128, max_keypoints 2048), config/config.yaml:44,53 (laf_to_sideinfo_method 'none' = response only, num_iters 20)
    "S128": dict(descriptor_dim=128, num_stages=9, num_heads=4, num_iters=20, side_info_size=1,
                 kpts=(2048, 2048), batch=32),
    # ... and for its 256-d family: config/features/superpoint_magicleap.yaml:2-4 (descriptor_dim 256, max_keypoints 2048), num_iters 20
    "S256": dict(descriptor_dim=256, num_stages=9, num_heads=4, num_iters=20, side_info_size=1,
                 kpts=(2048, 2048), batch=32),
    # BASELINE configs[3] leaves the Sinkhorn iteration count open: C4 runs 100 like configs[1-2]; this is the sibling at the reference's default 20
    "C4i20": dict(descriptor_dim=128, num_stages=9, num_heads=4, num_iters=20, side_info_size=6,
                  kpts=(4096, 4096), batch=8),
}


def make_config(descriptor_dim: int = 256, num_stages: int = 9, num_heads: int = 4,
                num_iters: int = 100, side_info_size: int = 1, reg: float = 1.0,
                residual: bool = True, use_offset: bool = False, no_descriptors: bool = False,
                dustbin_score_init: float = 1.0,
                hidden_layers_sizes: Sequence[int] = (32, 64, 128), encoder_name: str = "FeedForwardNet",
                attention: str = "softmax", **_unused) -> dict:
    """The `superglue:` config block with the keys SuperGlue.__init__ reads
    (reference models/superglue/superglue.py:16-27, config/config.yaml:42-55) plus the keys
    MatchingTrainingModule injects (models/matching_module.py:35-43)."""
    return {
        "descriptor_dim": descriptor_dim,
        "positional_encoding": {
            "output_size": descriptor_dim,
            "side_info_size": side_info_size,
            "encoder_name": encoder_name,
            "hidden_layers_sizes": list(hidden_layers_sizes),
        },
        "attention_gnn": {
            "num_stages": num_stages,
            "embed_dim": descriptor_dim,
            "num_heads": num_heads,
            "attention": attention,
            "use_offset": use_offset,
        },
        "dustbin_score_init": dustbin_score_init,
        "otp": {"num_iters": num_iters, "reg": reg},
        "residual": residual,
        "no_descriptors": no_descriptors,
    }


def state_dict_spec(config: dict) -> "OrderedDict[str, tuple]":
    """Names, shapes and kinds of every state-dict entry of the reference module
    (SURVEY.md §3.6), in the reference's registration order."""
    D = config["descriptor_dim"]
    pe = config["positional_encoding"]
    sizes = [2 + pe["side_info_size"], *pe["hidden_layers_sizes"], pe["output_size"]]
    L = config["attention_gnn"]["num_stages"]
    spec: "OrderedDict[str, tuple]" = OrderedDict()

    def conv(prefix, cout, cin):
        spec[prefix + ".weight"] = ((cout, cin, 1), "conv_w", cin)
        spec[prefix + ".bias"] = ((cout,), "conv_b", cin)

    def bn(prefix, c):
        spec[prefix + ".weight"] = ((c,), "bn_w", 0)
        spec[prefix + ".bias"] = ((c,), "bn_b", 0)
        spec[prefix + ".running_mean"] = ((c,), "bn_mean", 0)
        spec[prefix + ".running_var"] = ((c,), "bn_var", 0)
        spec[prefix + ".num_batches_tracked"] = ((), "bn_count", 0)

    if config.get("residual", False):
        spec["mix_coefs"] = ((D, 1), "mix", 0)
    spec["dustbin_score"] = ((), "dustbin", 0)
    if pe.get("encoder_name", "FeedForwardNet") == "FeedForwardNetSiren":
        # FeedForwardNetSiren = [Conv1d, Sine] * (n-1) + Conv1d (models/utils.py:32-45) -> conv indices 0, 2, 4, ...
        for i in range(1, len(sizes)):
            conv(f"positional_encoding.encoder.{2 * (i - 1)}", sizes[i], sizes[i - 1])
    else:
        # FeedForwardNet = [Conv1d, ReLU, BatchNorm1d] * (n-1) + Conv1d  -> Sequential indices 0,(1),2, 3,(4),5, ...
        idx = 0
        for i in range(1, len(sizes) - 1):
            conv(f"positional_encoding.encoder.{idx}", sizes[i], sizes[i - 1])
            bn(f"positional_encoding.encoder.{idx + 2}", sizes[i])
            idx += 3
        conv(f"positional_encoding.encoder.{idx}", sizes[-1], sizes[-2])
    favor = config["attention_gnn"].get("attention", "softmax") == "favor_relu"
    for l in range(2 * L):
        p = f"attention_gnn.layers.{l}.module"
        if favor:   # GeneralizedFavorAttention registers its random features as a buffer (attention.py:43-53; __init__.py:19-25:
            #         num_orthogonal_features = 2 * embed_dim), created before the projections (attention_gnn.py:14)
            spec[f"{p}.mha.attention_func.projection_matrix"] = ((2 * D, D), "favor_proj", D)
        for name in ("in_proj_q", "in_proj_k", "in_proj_v", "out_proj"):
            conv(f"{p}.mha.{name}", D, D)
        conv(f"{p}.fc.0", 2 * D, 2 * D)
        bn(f"{p}.fc.2", 2 * D)
        conv(f"{p}.fc.3", D, 2 * D)
    conv("linear_proj", D, D)
    return spec


def orthogonal_random_features(num_rows: int, num_cols: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """FAVOR+ random features as the reference draws them (FavorAttention.sample_orthogonal_random_vectors, attention.py:62-78):
    ceil(rows / cols) Gaussian blocks [cols, cols], each orthogonalised by QR, the unit rows rescaled by the norms of the
    Gaussian rows."""
    blocks = math.ceil(num_rows / num_cols)
    unstructured = torch.randn(blocks, num_cols, num_cols, generator=generator)
    norm = unstructured.norm(dim=-1).view(-1, 1)
    q, _ = torch.linalg.qr(unstructured, mode="reduced")
    q = q.transpose(-1, -2).reshape(-1, num_cols)
    return q[:num_rows] * norm[:num_rows]


def make_state_dict(config: dict, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic weights keyed by parameter NAME (not by module construction order), so the
    reference module, the oracle and the HIP module all see the same numbers.
    Conv weights/biases ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (PyTorch's default Conv1d init);
    BatchNorm affine/statistics randomised."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, (shape, kind, fan_in) in state_dict_spec(config).items():
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
        if kind in ("conv_w", "conv_b"):
            bound = 1.0 / math.sqrt(fan_in)
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif kind in ("bn_w", "bn_var"):
            t = 0.75 + 0.5 * torch.rand(shape, generator=g)
        elif kind in ("bn_b", "bn_mean"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif kind == "bn_count":
            t = torch.tensor(1, dtype=torch.long)
        elif kind == "mix":
            t = 0.5 * torch.randn(shape, generator=g)
        elif kind == "dustbin":
            t = torch.tensor(float(config["dustbin_score_init"]))
        elif kind == "favor_proj":
            t = orthogonal_random_features(shape[0], shape[1], g)
        else:  # pragma: no cover
            raise AssertionError(kind)
        out[name] = t
    return out


def make_trained_like_state_dict(config: dict, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """make_state_dict with the statistics a TRAINED checkpoint shows and random initialisation never does:
    in every message MLP a few BatchNorm channels are DEAD (post-ReLU output identically 0: running_mean = 0, running_var ~ 1e-12, so
    the eval-mode fold multiplies the next conv's column by ~316 * gamma), a few have a large gamma / sigma ratio, the matching conv
    columns carry ordinary weights, and a few projection weights are large.  Deterministic in (config, seed)."""
    sd = make_state_dict(config, seed)
    D = config["descriptor_dim"]
    L = 2 * config["attention_gnn"]["num_stages"]
    g = torch.Generator().manual_seed(977 + seed)
    for l in range(L):
        pre = f"attention_gnn.layers.{l}.module"
        dead = torch.randperm(2 * D, generator=g)[:3]
        sd[f"{pre}.fc.2.running_var"][dead] = 1e-12
        sd[f"{pre}.fc.2.running_mean"][dead] = 0.0
        sd[f"{pre}.fc.2.weight"][dead] = 8.0 + 4.0 * torch.rand(3, generator=g)
        sd[f"{pre}.fc.3.weight"][:, dead, 0] = 0.3 * torch.randn(D, 3, generator=g)          # 0.3 * 10 / sqrt(1e-5) * 256 >> 65504
        # a dead channel is dead because its conv row is strongly negative for every input: make it so (bias far below any response)
        sd[f"{pre}.fc.0.bias"][dead] = -1e3
        big = torch.randperm(2 * D, generator=g)[:4]
        sd[f"{pre}.fc.2.running_var"][big] = 1e-4            # gamma / sigma ~ 100
        if l % 3 == 0:
            sd[f"{pre}.mha.in_proj_k.weight"][l % D, (7 * l + 3) % D, 0] = 150.0                # 256 * 150 > 32768
    return sd


def make_pair(m: int, n: int, descriptor_dim: int, side_info_size: int, seed: int,
              desc_scale: float = 32.0, inlier_frac: float = 0.6) -> Dict[str, torch.Tensor]:
    """One synthetic image pair (no batch dimension)."""
    g = torch.Generator().manual_seed(1_000_003 * (seed + 1))
    W, H = IMAGE_WH
    wh = torch.tensor([W - 1.0, H - 1.0])
    k0 = torch.rand(m, 2, generator=g) * wh
    d0 = torch.nn.functional.normalize(torch.randn(m, descriptor_dim, generator=g), dim=-1)
    k1 = torch.rand(n, 2, generator=g) * wh
    d1 = torch.nn.functional.normalize(torch.randn(n, descriptor_dim, generator=g), dim=-1)
    n_in = min(int(inlier_frac * min(m, n)), m, n)
    src = torch.randperm(m, generator=g)[:n_in]
    dst = torch.randperm(n, generator=g)[:n_in]
    k1[dst] = (k0[src] + 2.0 * torch.randn(n_in, 2, generator=g)).clamp_(min=0.0)
    k1[dst] = torch.minimum(k1[dst], wh)
    d1[dst] = torch.nn.functional.normalize(
        d0[src] + 0.02 * torch.randn(n_in, descriptor_dim, generator=g), dim=-1)
    s0 = torch.rand(m, side_info_size, generator=g)
    s1 = torch.rand(n, side_info_size, generator=g)
    return {
        "keypoints0": k0, "keypoints1": k1,
        "local_descriptors0": d0 * desc_scale, "local_descriptors1": d1 * desc_scale,
        "side_info0": s0, "side_info1": s1,
    }


def make_batch(batch: int, m: int, n: int, descriptor_dim: int, side_info_size: int = 1,
               seed: int = 0, first_pair: int = 0, device: Optional[torch.device] = None,
               **pair_kw) -> Dict[str, object]:
    """A batch of `batch` pairs; pair p of the job uses seed (seed, first_pair + p) so that a
    sharded job sees the same pairs whatever the world size."""
    pairs = [make_pair(m, n, descriptor_dim, side_info_size, seed * 100_003 + first_pair + p, **pair_kw)
             for p in range(batch)]
    data: Dict[str, object] = {k: torch.stack([p[k] for p in pairs]) for k in pairs[0]}
    if device is not None:
        data = {k: v.to(device) for k, v in data.items()}
    data["image0_size"] = list(IMAGE_WH)  # [W, H]  (reference superglue.py:38 reverses it)
    data["image1_size"] = list(IMAGE_WH)
    return data


def ragged_lengths(batch: int, lo: int, hi: int, seed: int = 0) -> List[tuple]:
    """BASELINE config 5: per-image keypoint counts ~ U{lo..hi}."""
    g = torch.Generator().manual_seed(77_777 + seed)
    t = torch.randint(lo, hi + 1, (batch, 2), generator=g)
    return [(int(a), int(b)) for a, b in t.tolist()]


# ---------------------------------------------------------------- SuperPoint inputs (openglue_amd/superpoint.py)
def make_image(H: int, W: int, seed: int, shapes: int = 24, flat: bool = False) -> torch.Tensor:
    """[1, 1, H, W] in [0, 1]: filled convex polygons and ellipses of random grey levels over a grey background, blurred
    (Gaussian, sigma 1 px), with mild noise (sigma 0.01).  flat=True draws a few faint, large shapes and no noise: a sparse image."""
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    img = torch.full((H, W), 0.5 if flat else float(U(1)) * 0.6 + 0.2, dtype=torch.float64)
    n = 3 if flat else shapes
    for _ in range(n):
        cx, cy = float(U(1)) * W, float(U(1)) * H
        r = (0.25 + 0.35 * float(U(1))) * min(H, W) if flat else (0.04 + 0.16 * float(U(1))) * min(H, W)
        level = 0.5 + (float(U(1)) - 0.5) * 0.08 if flat else float(U(1))
        if float(U(1)) < 0.5:       # ellipse
            a, b, th = r, r * (0.3 + 0.7 * float(U(1))), float(U(1)) * math.pi
            u = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
            v = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
            inside = (u / a) ** 2 + (v / b) ** 2 <= 1.0
        else:                       # convex polygon: 3..7 vertices on a circle
            k = 3 + int(U(1) * 5)
            ang = torch.sort(U(k) * 2 * math.pi).values
            px, py = cx + r * torch.cos(ang), cy + r * torch.sin(ang)
            inside = torch.ones(H, W, dtype=torch.bool)
            for i in range(k):
                x0, y0, x1, y1 = float(px[i]), float(py[i]), float(px[(i + 1) % k]), float(py[(i + 1) % k])
                inside &= (x1 - x0) * (yy - y0) - (y1 - y0) * (xx - x0) >= 0
        img = torch.where(inside, torch.tensor(level, dtype=torch.float64), img)
    t = torch.arange(-3, 4, dtype=torch.float64)
    k1 = torch.exp(-t * t / 2.0)
    k1 = k1 / k1.sum()
    x = torch.nn.functional.pad(img[None, None], (3, 3, 3, 3), mode="replicate")
    x = torch.nn.functional.conv2d(x, k1.view(1, 1, 1, 7))
    x = torch.nn.functional.conv2d(x, k1.view(1, 1, 7, 1))
    x = x + (0.0 if flat else 0.01) * torch.randn(x.shape, generator=g, dtype=torch.float64)
    return x.clamp(0.0, 1.0).to(torch.float32)


def random_homography(H: int, W: int, seed: int, strength: float = 0.12) -> torch.Tensor:
    """[3, 3] float64 mapping pixel (x, y, 1) of image 0 to image 1: the image corners moved by up to strength * size."""
    g = torch.Generator().manual_seed(seed)
    src = torch.tensor([[0.0, 0.0], [W - 1.0, 0.0], [W - 1.0, H - 1.0], [0.0, H - 1.0]], dtype=torch.float64)
    dst = src + (torch.rand(4, 2, generator=g, dtype=torch.float64) - 0.5) * 2 * strength * torch.tensor([W, H], dtype=torch.float64)
    A = []
    for (x, y), (u, v) in zip(src.tolist(), dst.tolist()):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    _, _, vh = torch.linalg.svd(torch.tensor(A, dtype=torch.float64))
    Hm = vh[-1].view(3, 3)
    return Hm / Hm[2, 2]


def warp_image(image: torch.Tensor, Hm: torch.Tensor) -> torch.Tensor:
    """Second view of a pair: out(p) = image(Hm^-1 p), bilinear, border pixels replicated.  image [1, 1, H, W]."""
    _, _, H, W = image.shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    p = torch.stack([xx, yy, torch.ones_like(xx)], -1) @ torch.linalg.inv(Hm).T
    sx, sy = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    grid = torch.stack([sx / (W - 1) * 2 - 1, sy / (H - 1) * 2 - 1], -1)[None]
    out = torch.nn.functional.grid_sample(image.to(torch.float64), grid, mode="bilinear", padding_mode="border", align_corners=True)
    return out.to(torch.float32)


def make_superpoint_state_dict(batch_norm: bool = False, seed: int = 0, descriptor_dim: int = 256) -> "OrderedDict[str, torch.Tensor]":
    """Seeded SuperPoint weights with a realistic heatmap.  PyTorch's default init collapses the 65-way softmax to ~1/65
    everywhere (every NMS decision a near-tie); here the trunk is He-normal and convPb is scaled up so that the detector's
    logits spread over several units.  With batch_norm the BatchNorm affine parameters and running statistics are randomised
    around the identity."""
    g = torch.Generator().manual_seed(seed)
    chans = [(1, 64), (64, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128), (128, 128)]
    names = [f"conv{i}{s}" for i in range(1, 5) for s in "ab"]
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    convs = list(zip(names, chans, [3] * 8)) + [("convPa", (128, 256), 3), ("convPb", (256, 65), 1),
                                                ("convDa", (128, 256), 3), ("convDb", (256, descriptor_dim), 1)]
    for name, (cin, cout), k in convs:
        std = math.sqrt(2.0 / (cin * k * k))
        if name == "convPb":
            std *= 6.0
        sd[f"{name}.weight"] = torch.randn(cout, cin, k, k, generator=g) * std
        sd[f"{name}.bias"] = torch.randn(cout, generator=g) * 0.01
    if batch_norm:
        bns = [(f"bn{i}{s}", c) for i, (s, c) in zip([1, 1, 2, 2, 3, 3, 4, 4], [("a", 64), ("b", 64)] * 2 + [("a", 128), ("b", 128)] * 2)]
        bns += [("bnPa", 256), ("bnPb", 65), ("bnDa", 256), ("bnDb", descriptor_dim)]
        for name, c in bns:
            sd[f"{name}.weight"] = 0.8 + 0.4 * torch.rand(c, generator=g)
            sd[f"{name}.bias"] = torch.randn(c, generator=g) * 0.05
            sd[f"{name}.running_mean"] = torch.randn(c, generator=g) * 0.05
            sd[f"{name}.running_var"] = 0.8 + 0.4 * torch.rand(c, generator=g)
            sd[f"{name}.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


# ---------------------------------------------------------------- patch networks (openglue_amd/affnet_hardnet.py)
def make_patchnet_state_dict(kind: str, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded HardNet / AffNet / OriNet weights in kornia's state-dict layout (`features.{i}.*`): convolutions with PyTorch's default
    init (uniform in +-1 / sqrt(fan_in), weights and the bias of features.19), BatchNorm running_mean ~ N(0, 0.1^2) and running_var ~
    U(0.75, 1.25), so that no BatchNorm is an identity."""
    if kind not in ("hardnet", "affnet", "orinet"):
        raise ValueError(f"kind must be hardnet, affnet or orinet, got {kind!r}")
    g = torch.Generator().manual_seed(1000 * seed + {"hardnet": 1, "affnet": 2, "orinet": 3}[kind])
    c = 32 if kind == "hardnet" else 16
    nout = {"hardnet": 128, "affnet": 3, "orinet": 2}[kind]
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()

    def conv(i, cout, cin, k, bias):
        bound = 1.0 / math.sqrt(cin * k * k)
        sd[f"features.{i}.weight"] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        if bias:
            sd[f"features.{i}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound

    def bn(i, ch):
        sd[f"features.{i}.running_mean"] = torch.randn(ch, generator=g) * 0.1
        sd[f"features.{i}.running_var"] = 0.75 + 0.5 * torch.rand(ch, generator=g)
        sd[f"features.{i}.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)

    for i, (cin, cout) in zip((0, 3, 6, 9, 12, 15), [(1, c), (c, c), (c, 2 * c), (2 * c, 2 * c), (2 * c, 4 * c), (4 * c, 4 * c)]):
        conv(i, cout, cin, 3, False)
        bn(i + 1, cout)
    conv(19, nout, 4 * c, 8, kind != "hardnet")
    if kind == "hardnet":
        bn(20, 128)
    return sd
