"""mms2ut-extract-image-features: the reference's mm_s2ut/scripts/extract_feature/get_img_feat_vit.py on
the HIP ViT (multimodal-s2ut_amd/vision.py): the images of a Multi30k split in, one fp32 [N, 577, d]
``.pth`` of ViT features out, the image input of training and inference (manifest.ImageFeatures).

    python scripts/mms2ut_extract_image_features.py --dataset train --path /data/multi30k \\
        --model vit_base_patch16_384 --checkpoint-path vit_base_patch16_384.pth --save-dir feats/vit_base

--path holds the list files (train.txt, val.txt, test_2016_flickr.txt, test_2017_flickr.txt,
test_2017_mscoco.txt; the file name is the text before the first '#' of a line) and the image directories
(flickr30k-images, test2017-images, testcoco-images).  --checkpoint-path is a timm-layout state dict:
torch.save'd (also wrapped in 'state_dict' or 'model') or .safetensors.  The output is train / valid / test /
test1 / test2 .pth under --save-dir.  Images are decoded with PIL on --num-workers threads while the
device works on the previous batch; resize, crop, normalisation and the ViT run on the device."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", required=True, choices=["train", "val", "test2016", "test2017", "testcoco"])
    ap.add_argument("--path", required=True, help="directory of the list files and the *-images directories")
    ap.add_argument("--model", required=True, help="vit_{tiny,small,base,large}_patch16_384, vit_base_patch16_clip_384[.laion2b_ft_in12k_in1k]")
    ap.add_argument("--checkpoint-path", required=True, help="timm-layout state dict (.pth / .bin / .safetensors)")
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--batch-size", type=int, default=32, help="images per device batch")
    ap.add_argument("--num-workers", type=int, default=8, help="decode threads")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.num_workers < 1:
        ap.error("--batch-size and --num-workers must be >= 1")
    V = importlib.import_module("multimodal-s2ut_amd.vision")
    model = V.ViTFeatures.from_checkpoint(args.model, args.checkpoint_path, args.device)
    path, shape = V.extract_dataset(model, args.path, args.dataset, args.save_dir, args.batch_size, args.num_workers,
                                    V.print_progress)
    print(f"feature shape: {shape}, saved in: {path}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
