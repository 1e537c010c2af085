"""mms2ut-transcript: the reference's mm_s2ut/scripts/transcript.py on the HIP wav2vec2 (the pipeline's
ASR step, between the vocoder and BLEU): synthesized WAV files in, one transcript per line out.

    python scripts/mms2ut_transcript.py --model-path wav2vec2-large-960h-lv60-self/ \\
        --tts-wav-dir out/ --transcript-txt transcript.txt

--model-path is an HF model directory (config.json, vocab.json, model.safetensors or
pytorch_model.bin).  The files of --tts-wav-dir ({i}_pred.wav, as mms2ut_generate_waveform.py writes
them) are taken in the order of the integer before the first '_'; the transcripts are joined by
newlines without a trailing one."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model-path", required=True, help="HF Wav2Vec2ForCTC model directory")
    ap.add_argument("--tts-wav-dir", required=True, help="directory of {i}_pred.wav (16 kHz, 16-bit PCM)")
    ap.add_argument("--transcript-txt", required=True, help="output file, one transcript per line")
    ap.add_argument("--batch-size", type=int, default=8, help="utterances per encoder batch")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    A = importlib.import_module("multimodal-s2ut_amd.asr")
    model = A.Wav2Vec2CTC.from_pretrained(args.model_path, args.device)
    n = A.transcribe_dir(model, args.tts_wav_dir, args.transcript_txt, args.batch_size)
    print(f"transcribed {n} files to {args.transcript_txt}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
