"""mms2ut-quantize-units: fairseq's examples/textless_nlp/gslm/speech2unit/clustering/quantize_with_kmeans.py
(the reference's scripts/preprocess/3_cluster.sh) on the HIP HuBERT: speech in, k-means units out.

    python scripts/mms2ut_quantize_units.py --feature_type hubert --acoustic_model_path mhubert_base/ \\
        --kmeans_model_path mhubert_base_vp_en_es_fr_it3_L11_km1000.bin --layer 11 \\
        --manifest_path train.tsv --out_quantized_file_path train.km --extension .wav

--acoustic_model_path is an HF model directory (config.json, model.safetensors or pytorch_model.bin,
optionally preprocessor_config.json); fairseq's .pt checkpoints are not read.  --kmeans_model_path is a
joblib-pickled scikit-learn k-means or a .npy file of its cluster_centers_.  The manifest is fairseq's: the
root directory on the first line, then ``relative/path<TAB>n_samples``.  One line per file comes out, in
manifest order: ``{basename without extension}|{units joined by spaces}``; --reduce collapses runs of
equal units.  --beamsearch [--top_k 10] [--beamsize 200] writes the units of the reference's own decode
(scripts/speech_to_speech_translation/mhubert.py, beamsearch=True) instead: a length-penalised beam search
over each frame's top_k nearest centroids."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--feature_type", required=True, help="only 'hubert'")
    ap.add_argument("--acoustic_model_path", required=True, help="HF HubertModel directory")
    ap.add_argument("--kmeans_model_path", required=True, help="joblib k-means model or .npy centroids [Kc, d]")
    ap.add_argument("--layer", type=int, required=True, help="hidden_states index the k-means was trained on")
    ap.add_argument("--manifest_path", required=True)
    ap.add_argument("--out_quantized_file_path", required=True)
    ap.add_argument("--extension", default=".wav", help="stripped from the file names in the output")
    ap.add_argument("--batch-size", type=int, default=8, help="utterances per encoder batch")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--reduce", action="store_true", help="write the units with runs collapsed")
    ap.add_argument("--beamsearch", action="store_true",
                    help="write the reference's beam decode (mhubert.py HubertCode.decode) instead of the nearest centroids")
    ap.add_argument("--top_k", type=int, default=10, help="with --beamsearch: nearest centroids per frame (at most 32)")
    ap.add_argument("--beamsize", type=int, default=200,
                    help="with --beamsearch: sequences kept per frame (beamsize x top_k at most 2048)")
    args = ap.parse_args(argv)
    if args.feature_type != "hubert":
        ap.error(f"--feature_type '{args.feature_type}' is not supported (only 'hubert')")
    if args.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    if not os.path.isdir(args.acoustic_model_path):
        ap.error(f"--acoustic_model_path '{args.acoustic_model_path}' is not a directory: an HF model directory is "
                 "expected; fairseq's .pt checkpoint format is out of scope (convert it to the HF layout first)")
    U = importlib.import_module("multimodal-s2ut_amd.units")
    model = U.HubertUnits.from_pretrained(args.acoustic_model_path, args.kmeans_model_path, args.layer, args.device)
    n = U.quantize_manifest(model, args.manifest_path, args.out_quantized_file_path, args.extension, args.batch_size,
                            args.reduce, args.beamsearch, args.top_k, args.beamsize)
    print(f"quantised {n} files to {args.out_quantized_file_path}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
