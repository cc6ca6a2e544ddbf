"""Two images to verified matches on the GPU: SuperPointNetBn (or SIFT) -> OpenGlueMatcher(SuperGlue) -> find_fundamental, the whole
of the reference's inference.py run_inference, on a synthetic homography pair with seeded weights.  Prints the shapes and the time per stage.
The pair is related by a homography, which is degenerate for a fundamental matrix (a family of F fits it equally well): the inlier
count is shown, the accuracy of the stage is the business of tests/test_gpu_geometry.py.

    python examples/match_images.py [--size 480x640] [--keypoints 2048] [--match-threshold 0.2] [--features {superpoint,sift,dog_affnet_hardnet}]
                                    [--verify {fundamental,homography}] [--scoring {inliers,sigma}]

--verify homography runs find_homography (cv2.findHomography(..., cv2.RANSAC, 3.0)) as the last stage instead, the model that fits
this planar pair, and prints its inliers and the mean corner error against the homography the pair was made with.

--scoring sigma scores the last stage by MAGSAC++'s sigma-consensus with weighted refits (geometry.py), which is what the reference's
cv2.USAC_MAGSAC does; the default counts inliers.

--features sift runs the reference's 128-d pipeline: the SIFT extractor (openglue_amd/sift.py) and a 128-d SuperGlue.
--features dog_affnet_hardnet runs DoG + AffNet + OriNet + HardNet (openglue_amd/affnet_hardnet.py, seeded weights) with the affine
LAF side information: laf_to_sideinfo_method "affine", side_info_size 6.

The seeded weights are not trained: at the reference's threshold of 0.2 they may leave no match at all, and the last stage then
times its four launches on an empty pair.  --match-threshold 0 keeps every mutual best match and gives the stage real work.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.openglue_matcher import OpenGlueMatcher  # noqa: E402
from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.affnet_hardnet import DoGAffNetHardNet  # noqa: E402
from openglue_amd.geometry import find_fundamental, find_homography  # noqa: E402
from openglue_amd.metrics import homography_error  # noqa: E402
from openglue_amd.sift import SIFT  # noqa: E402
from openglue_amd.superglue import SuperGlue  # noqa: E402
from openglue_amd.superpoint import SuperPointNetBn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--match-threshold", type=float, default=0.2)
    ap.add_argument("--features", choices=("superpoint", "sift", "dog_affnet_hardnet"), default="superpoint")
    ap.add_argument("--verify", choices=("fundamental", "homography"), default="fundamental")
    ap.add_argument("--scoring", choices=("inliers", "sigma"), default="inliers")
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    dev = torch.device("cuda:0")
    img0 = syn.make_image(H, W, seed=1)
    Hm = syn.random_homography(H, W, seed=2)
    img1 = syn.warp_image(img0, Hm)
    find = find_homography if a.verify == "homography" else find_fundamental
    verify = (lambda k0, k1: find(k0, k1, scoring="sigma")) if a.scoring == "sigma" else find
    affine = a.features == "dog_affnet_hardnet"
    if a.features == "sift":
        sp = SIFT(max_keypoints=a.keypoints).to(dev)
    elif affine:
        sp = DoGAffNetHardNet(max_keypoints=a.keypoints)
        sp.hardnet.load_state_dict(syn.make_patchnet_state_dict("hardnet", seed=1))
        sp.affnet.load_state_dict(syn.make_patchnet_state_dict("affnet", seed=1))
        sp.orinet.angle_detector.load_state_dict(syn.make_patchnet_state_dict("orinet", seed=1))
        sp = sp.eval().to(dev)
    else:
        sp = SuperPointNetBn(max_keypoints=a.keypoints, keypoint_threshold=0.005)
        sp.load_state_dict(syn.make_superpoint_state_dict(True, seed=1))
        sp = sp.eval().to(dev)
    cfg = syn.make_config(descriptor_dim=256 if a.features == "superpoint" else 128, num_stages=9, num_heads=4, num_iters=20,
                          side_info_size=6 if affine else 1)
    sg = SuperGlue(cfg).eval()
    sg.load_state_dict(syn.make_state_dict(cfg, seed=0))
    sg = sg.to(dev)
    matcher = OpenGlueMatcher(sp, sg, {"superglue": {"laf_to_sideinfo_method": "affine" if affine else "none"}, "inference": {"match_threshold": a.match_threshold}})
    data = {"image0": img0.to(dev), "image1": img1.to(dev)}
    for _ in range(2):                      # warm-up: packing, allocator
        out = matcher(data)
        verify(out["keypoints0"], out["keypoints1"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lafs, _, _ = sp(torch.cat([data["image0"], data["image1"]]))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = matcher(data)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    F, inliers = verify(out["keypoints0"], out["keypoints1"])      # cv2.findFundamentalMat(..., USAC_MAGSAC, 1.0, 0.999, 100000) / cv2.findHomography
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"{H}x{W}: {lafs.shape[1]} keypoints per image, {out['keypoints0'].shape[0]} matches")
    print(f"{ {'sift': 'SIFT', 'superpoint': 'SuperPoint', 'dog_affnet_hardnet': 'DoG + AffNet + OriNet + HardNet'}[a.features]} on both images {1e3 * (t1 - t0):.2f} ms; images -> matches {1e3 * (t2 - t1):.2f} ms")
    if a.verify == "homography":
        err = float(homography_error(F[None], torch.as_tensor(Hm, dtype=torch.float32, device=dev).reshape(1, 3, 3), (W, H))[0])
        print(f"homography: {int(inliers.sum())} inliers of {inliers.shape[0]} matches, mean corner error {err:.2f} px, {1e3 * (t3 - t2):.2f} ms")
    else:
        print(f"fundamental matrix: {int(inliers.sum())} inliers of {inliers.shape[0]} matches, {1e3 * (t3 - t2):.2f} ms")


if __name__ == "__main__":
    main()
