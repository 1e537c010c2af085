"""mms2ut-resample: the reference's scripts/preprocess/1_preprocess.ipynb (`ffmpeg -ar 16000` over the corpus)
on the HIP resampler: every *.wav under SRC, recursively, to 16-bit mono RATE Hz at the same path under DST.

    python scripts/mms2ut_resample.py speech/wav/es speech/16khz_wav/es

The filter is bandlimited sinc interpolation with torchaudio's "kaiser_best" parameters (multimodal-s2ut_amd/
prepare.py); it is not bit-equal to ffmpeg's swresample.  Sources are 16-bit PCM WAV at any rate, channels
averaged to mono; files already mono at RATE are copied as they are (a tree of only such files needs no GPU).
Other sample formats and compressed audio (mp3) are refused by name: decode them to 16-bit PCM first."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src", metavar="SRC", help="directory searched recursively for *.wav")
    ap.add_argument("dst", metavar="DST", help="output directory (relative paths are kept)")
    ap.add_argument("--rate", type=int, default=16000, help="output sample rate in Hz")
    ap.add_argument("--batch-size", type=int, default=64, help="clips per kernel launch")
    ap.add_argument("--num-workers", type=int, default=8, help="threads that read and write WAV files")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.rate < 1 or args.batch_size < 1 or args.num_workers < 1:
        ap.error("--rate, --batch-size and --num-workers must be >= 1")
    if not os.path.isdir(args.src):
        ap.error(f"SRC '{args.src}' is not a directory")
    if os.path.realpath(args.src) == os.path.realpath(args.dst):
        ap.error("DST must differ from SRC (files are written at the same relative paths)")
    P = importlib.import_module("multimodal-s2ut_amd.prepare")
    rep = P.convert_dir(args.src, args.dst, args.rate, args.batch_size, args.num_workers, args.device)
    by_rate = ", ".join(f"{n} from {sr} Hz" for sr, n in sorted(rep["resampled"].items())) or "none"
    print(f"converted {rep['files']} files to {args.rate} Hz mono under {args.dst}: {rep['copied']} copied, "
          f"resampled {by_rate}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
