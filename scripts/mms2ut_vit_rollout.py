"""mms2ut-vit-rollout: the reference's mm_s2ut/scripts/extract_feature/vit_rollout.py on the HIP ViT
(multimodal-s2ut_amd/vision.py ViTFeatures.rollout): images in, one fp32 [N, S/P, S/P] ``.pth`` of attention
rollout masks out -- per image the regions the class token draws on, divided by their maximum.

    python scripts/mms2ut_vit_rollout.py --dataset val --path /data/multi30k \\
        --model vit_base_patch16_384 --checkpoint-path vit_base_patch16_384.pth --save-dir rollout/vit_base
    python scripts/mms2ut_vit_rollout.py --image a.jpg b.jpg --model ... --checkpoint-path ... --save-dir out \\
        --overlay-dir out/png

Images come from --dataset / --path (the feature extractor's Multi30k conventions; the output is train / valid /
test / test1 / test2 _rollout.pth) or from --image FILE... (the output is {--name}_rollout.pth, "images" by
default).  --head-fusion, --discard-ratio: the reference's head_fusion and discard_ratio.  --normalization
reference reproduces the reference's a / a.sum(-1), which divides column j by row j's sum; row is the row
normalisation of Abnar & Zuidema.  --overlay-dir also writes one PNG per image, the mask resized to the image
and blended over it (presentation only, on the host).  Images are decoded with PIL on --num-workers threads."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", choices=["train", "val", "test2016", "test2017", "testcoco"])
    ap.add_argument("--path", help="directory of the list files and the *-images directories (with --dataset)")
    ap.add_argument("--image", nargs="+", metavar="FILE", help="image files, instead of --dataset / --path")
    ap.add_argument("--name", default="images", help="output name with --image")
    ap.add_argument("--model", required=True, help="a vision.MODELS or vision.PRE_NORM_MODELS name")
    ap.add_argument("--checkpoint-path", required=True, help="timm-layout state dict (.pth / .bin / .safetensors)")
    ap.add_argument("--head-fusion", default="mean", choices=["mean", "max", "min"])
    ap.add_argument("--discard-ratio", type=float, default=0.9)
    ap.add_argument("--normalization", default="reference", choices=["reference", "row"])
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--overlay-dir", help="also write {image}_rollout.png overlays here")
    ap.add_argument("--batch-size", type=int, default=8, help="images per device batch")
    ap.add_argument("--num-workers", type=int, default=8, help="decode threads")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.num_workers < 1:
        ap.error("--batch-size and --num-workers must be >= 1")
    if not 0.0 <= args.discard_ratio <= 1.0:
        ap.error("--discard-ratio must be in [0, 1]")
    if bool(args.image) == bool(args.dataset):
        ap.error("give either --dataset with --path, or --image FILE...")
    if args.dataset and not args.path:
        ap.error("--dataset needs --path")
    V = importlib.import_module("multimodal-s2ut_amd.vision")
    try:
        V.model_config(args.model)
    except (ValueError, NotImplementedError) as e:
        ap.error(str(e))
    import torch
    if args.dataset:
        image_dir, listing, name = V.dataset_paths(args.path, args.dataset)
        paths = [os.path.join(image_dir, f) for f in V.read_list(listing)]
    else:
        paths, name = list(args.image), args.name
    model = V.ViTFeatures.from_checkpoint(args.model, args.checkpoint_path, args.device)
    masks = V.rollout_files(model, paths, args.batch_size, args.num_workers, args.head_fusion, args.discard_ratio,
                            args.normalization, args.overlay_dir, V.print_progress)
    os.makedirs(args.save_dir, exist_ok=True)
    out = os.path.join(args.save_dir, name + "_rollout.pth")
    torch.save(masks, out)
    print(f"rollout shape: {tuple(masks.shape)}, saved in: {out}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
