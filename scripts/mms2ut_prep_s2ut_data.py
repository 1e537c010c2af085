"""mms2ut-prep-s2ut-data: fairseq's examples/speech_to_speech/preprocessing/prep_s2ut_data.py as the reference
calls it (scripts/preprocess/5_prep_s2ut_data.sh): the {split}.tsv and config.yaml that mms2ut_train.py DATA reads.

    python scripts/mms2ut_prep_s2ut_data.py --source-dir speech/16khz_wav/es --target-dir manifest/train.es \\
        --data-split train --output-root format_data/es-en --reduce-unit \\
        --vocoder-checkpoint vocoder/model.pt --vocoder-cfg vocoder/config.json

Per split S: sources SOURCE_DIR/S/*.wav (16 kHz, in natural numeric order of the file names) and units
TARGET_DIR/S.txt (``id|u u u`` lines, mms2ut_quantize_units.py's output) -> OUTPUT_ROOT/S.tsv with the
columns id, src_audio, src_n_frames (samples // 160), tgt_text, tgt_n_frames.  The unit column is tgt_text,
the name the reference's dataset reads (stock fairseq writes tgt_audio).  Sources without units are skipped
and counted.  config.yaml: 80-bin fbank, utterance CMVN, the "lb" SpecAugment policy for training splits and
the code_hifigan vocoder entry."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--source-dir", required=True, help="source audio: SOURCE_DIR/SPLIT/*.wav, 16 kHz")
    ap.add_argument("--target-dir", required=True, help="target units: TARGET_DIR/SPLIT.txt")
    ap.add_argument("--data-split", required=True, nargs="+", metavar="S", help="splits to process")
    ap.add_argument("--output-root", required=True, help="directory for SPLIT.tsv and config.yaml")
    ap.add_argument("--reduce-unit", action="store_true", help="merge runs of equal units")
    ap.add_argument("--vocoder-checkpoint", required=True, help="written into config.yaml")
    ap.add_argument("--vocoder-cfg", required=True, help="written into config.yaml")
    args = ap.parse_args(argv)
    P = importlib.import_module("multimodal-s2ut_amd.prepare")
    rep = P.prep_s2ut_data(args.source_dir, args.target_dir, args.data_split, args.output_root, args.reduce_unit,
                           args.vocoder_checkpoint, args.vocoder_cfg)
    for line in P.report_lines(rep):
        print(line, file=sys.stderr)
    print(f"wrote {', '.join(s + '.tsv' for s in rep)} and config.yaml to {args.output_root}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
