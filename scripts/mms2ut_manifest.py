"""mms2ut-manifest: fairseq's examples/wav2vec/wav2vec_manifest.py --valid-percent 0 (the reference's
scripts/preprocess/2_manifest.sh): the manifest that mms2ut_quantize_units.py --manifest_path reads.

    python scripts/mms2ut_manifest.py speech/16khz_wav/es/train --dest manifest/train.es --ext wav

DEST/NAME.tsv gets the absolute ROOT on its first line, then ``relative/path<TAB>n_samples`` for every file
under ROOT (recursively) that ends in EXT, sample counts read from the WAV headers, in sorted order."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("root", metavar="ROOT", help="directory searched recursively")
    ap.add_argument("--dest", required=True, metavar="DIR", help="output directory")
    ap.add_argument("--ext", default="wav", help="file extension to look for")
    ap.add_argument("--name", default="train", help="the manifest is DIR/NAME.tsv (fairseq writes train.tsv)")
    args = ap.parse_args(argv)
    if not os.path.isdir(args.root):
        ap.error(f"ROOT '{args.root}' is not a directory")
    P = importlib.import_module("multimodal-s2ut_amd.prepare")
    path = os.path.join(args.dest, args.name + ".tsv")
    n = P.write_manifest(args.root, path, args.ext)
    print(f"wrote {n} files to {path}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
