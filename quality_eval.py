"""Fidelity and diversity of a folder of samples against real images: improved precision / recall, density / coverage and KID.

    python quality_eval.py --real DIR|DATASET --fake DIR [--features inception|pixels] [--k 5] [--kid [--kid_subsets 100]
                           [--kid_subset_size 1000]] [--n N] [--dataset_path datasets] [--output_dir DIR] [--seed 0] [--gpu 0]

FID is one number and cannot tell samples that got worse (fidelity: precision, density) from samples that collapsed onto fewer modes
(diversity: recall, coverage); KID is the unbiased alternative at small sample counts.  Definitions, arithmetic and the `<=` convention:
baddiffusion_amd/metrics.py (prdc, kid) and DESIGN.md section 3; the pairwise work runs in the HIP strip kernels of csrc/quality.hip.
  --real            a folder of images, or the name of a dataset (MNIST, CIFAR10, CELEBA, CELEBA-HQ) read through DatasetLoader from
                    --dataset_path; --fake is always a folder.  Both sets must have the same image size.
  --features        inception: the pool3 features FID uses (pytorch_fid's weights, BD_FID_WEIGHTS: a third-party asset; without it
                    this mode stops with an error).  pixels: the uint8 images / 255, flattened -- needs no asset and makes the whole
                    path runnable anywhere, but PIXEL-SPACE MANIFOLDS ARE CRUDE: Euclidean distance between raw images follows
                    brightness and alignment, not content.  Use it to test the plumbing or to compare runs of one model, not to
                    quote a number.
  --k               the k of the k-NN radii (1 ... 16; Naeem et al. use 5, Kynkaanniemi et al. 3)
  --kid             also KID: mean and standard deviation over --kid_subsets subsets of --kid_subset_size rows (capped at the smaller
                    set; the cap is recorded as KID_warning), drawn from a generator seeded with --seed
  --n               use the first N images of each set only
Output: <output_dir>/quality.json with "features", "n_real", "n_fake", "dim", "precision", "recall", "density", "coverage", "PRDC_k"
and, with --kid, "KID_mean", "KID_std", "KID_subsets", "KID_subset_size"[, "KID_warning"].
"""
import argparse
import json
import os

import numpy as np
import torch

FEATURES = ("inception", "pixels")


def get_config(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--real", type=str, required=True, help="folder of real images, or a dataset name")
    p.add_argument("--fake", type=str, required=True, help="folder of generated images")
    p.add_argument("--features", type=str, choices=FEATURES, default="inception",
                   help="inception: FID's pool3 features (needs the weights).  pixels: raw pixels / 255 -- no asset needed, but pixel-space "
                        "manifolds are crude (distance follows brightness and alignment, not content)")
    p.add_argument("--k", type=int, default=5)
    p.add_argument("--kid", action="store_true")
    p.add_argument("--kid_subsets", type=int)
    p.add_argument("--kid_subset_size", type=int)
    p.add_argument("--n", type=int, help="use the first N images of each set")
    p.add_argument("--dataset_path", "-dp", type=str, default="datasets")
    p.add_argument("--output_dir", "-od", type=str, default=".")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--gpu", "-g", type=str, default="0")
    args = p.parse_args(argv)
    if not 1 <= args.k <= 16:
        p.error(f"--k {args.k} must be in [1, 16]")
    if (args.kid_subsets is not None or args.kid_subset_size is not None) and not args.kid:
        p.error("--kid_subsets / --kid_subset_size need --kid")
    if (args.kid_subsets is not None and args.kid_subsets < 1) or (args.kid_subset_size is not None and args.kid_subset_size < 2):
        p.error("--kid_subsets must be at least 1 and --kid_subset_size at least 2")
    if args.n is not None and args.n < 2:
        p.error("--n must be at least 2")
    if not os.path.isdir(args.fake):
        p.error(f"--fake {args.fake} is not a folder")
    return args


def image_dir_u8(path, n=None):
    """the images of a folder (numeric file names in numeric order, others by name) as one uint8 [N, H, W, 3] array"""
    from PIL import Image

    def order(name):
        stem = os.path.splitext(name)[0]
        return (0, int(stem), "") if stem.isdigit() else (1, 0, name)
    files = sorted((f for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp"))), key=order)[:n]
    if len(files) < 2:
        raise ValueError(f"{path}: at least two images are needed, found {len(files)}")
    return np.stack([np.asarray(Image.open(os.path.join(path, f)).convert("RGB"), dtype=np.uint8) for f in files])


def real_u8(args, size, device):
    """the real set as a uint8 [N, H, W, 3] device tensor: a folder, or the first --n rows of a dataset at the fake images' size"""
    if os.path.isdir(args.real):
        return torch.from_numpy(image_dir_u8(args.real, args.n)).to(device)
    from baddiffusion_amd.dataset import DatasetLoader
    root = args.dataset_path if args.dataset_path and os.path.isdir(str(args.dataset_path)) else None
    channel = 1 if args.real == DatasetLoader.MNIST else 3
    dsl = DatasetLoader(root=root, name=args.real, channel=channel, image_size=size, seed=args.seed, device=device, num_images=args.n)
    imgs = dsl.device_images if args.n is None else dsl.device_images[: args.n]
    return imgs.expand(-1, -1, -1, 3).contiguous() if imgs.shape[-1] == 1 else imgs


def features_of(kind, images_u8, batch=500):
    """[N, d] float32 device features of a uint8 [N, H, W, 3] device tensor"""
    if kind == "pixels":
        return images_u8.reshape(images_u8.shape[0], -1).float() / 255.0
    from baddiffusion_amd import metrics
    from baddiffusion_amd.inception import load_fid_weights
    net = load_fid_weights(device=images_u8.device)
    if net is None:
        raise RuntimeError("--features inception needs pytorch_fid's InceptionV3 pool3 weights (point BD_FID_WEIGHTS at "
                           "pt_inception-2015-12-05-6726825d.pth); --features pixels needs no asset")
    store = metrics.FeatureStore(images_u8.shape[0])
    for s in range(0, images_u8.shape[0], batch):
        store.update(net(images_u8[s:s + batch]))
    return store.features()


def main(argv=None):
    args = get_config(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("quality_eval.py: a GPU is required (the pairwise kernels are HIP kernels; no CPU fallback)")
    device = torch.device("cuda", int(str(args.gpu).split(",")[0]))
    torch.cuda.set_device(device)
    from baddiffusion_amd import metrics
    fake = torch.from_numpy(image_dir_u8(args.fake, args.n)).to(device)
    real = real_u8(args, fake.shape[1], device)
    if real.shape[1:] != fake.shape[1:]:
        raise ValueError(f"image sizes differ: real {tuple(real.shape[1:])}, fake {tuple(fake.shape[1:])}")
    if args.k > min(real.shape[0], fake.shape[0]) - 1:
        raise ValueError(f"--k {args.k} needs more than {args.k} images in each set (real {real.shape[0]}, fake {fake.shape[0]})")
    fr, ff = features_of(args.features, real), features_of(args.features, fake)
    kid = {"subsets": args.kid_subsets or 100, "subset_size": args.kid_subset_size or 1000} if args.kid else None
    result = {"features": args.features, "n_real": int(fr.shape[0]), "n_fake": int(ff.shape[0]), "dim": int(fr.shape[1])}
    result.update(metrics.quality_scores(fr, ff, args.k, kid, generator=torch.Generator().manual_seed(args.seed)))
    os.makedirs(args.output_dir, exist_ok=True)
    with open(os.path.join(args.output_dir, "quality.json"), "w") as f:
        json.dump(result, f, indent=2, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
