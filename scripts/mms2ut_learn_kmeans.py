"""mms2ut-learn-kmeans: fairseq's examples/textless_nlp/gslm/speech2unit/clustering/cluster_kmeans.py on HIP
kernels -- the unit codebook that mms2ut_quantize_units.py (3_cluster.sh) then applies.

    python scripts/mms2ut_learn_kmeans.py --num_clusters 1000 --feature_type hubert \\
        --checkpoint_path hf_mhubert_dir --layer 11 --manifest_path train.tsv \\
        --out_kmeans_model_path km1000.npy --sample_pct 0.1

HuBERT features (HF HubertModel directory; fairseq's .pt checkpoints are not read) of a sampled share of the
manifest, or a .npy of features given with --features_path, then scikit-learn's MiniBatchKMeans.fit with
fairseq's settings on the device (multimodal-s2ut_amd/kmeans.py).  --out_kmeans_model_path *.npy holds the
centroids; any other suffix a joblib pickle of a scikit-learn MiniBatchKMeans (needs joblib and scikit-learn).
The published script is not part of this repository: its flag names are restated from fairseq's documentation
and are not pinned by a test against it."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _none_or_int(s):
    return None if s.lower() == "none" else int(s)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--num_clusters", type=int, required=True)
    ap.add_argument("--feature_type", required=True, help="only 'hubert'")
    ap.add_argument("--checkpoint_path", "--acoustic_model_path", dest="checkpoint_path", help="HF HubertModel directory")
    ap.add_argument("--layer", type=int, help="hidden_states index to cluster")
    ap.add_argument("--manifest_path")
    ap.add_argument("--out_kmeans_model_path", required=True, help="*.npy: centroids; otherwise a joblib scikit-learn model")
    ap.add_argument("--sample_pct", type=float, default=1.0, help="share of the manifest's files to use")
    ap.add_argument("--features_path", help=".npy of features [frames, d] in place of a model and a manifest")
    ap.add_argument("--out_features_path", help="also save the features (fp16 .npy)")
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--init", default="k-means++")
    ap.add_argument("--max_iter", type=int, default=150)
    ap.add_argument("--batch_size", type=int, default=10000, help="rows per mini-batch step")
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--max_no_improvement", type=_none_or_int, default=100, help="an integer or 'none'")
    ap.add_argument("--n_init", type=int, default=20)
    ap.add_argument("--reassignment_ratio", type=float, default=0.0)
    ap.add_argument("--extension", default=".wav")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.feature_type != "hubert":
        ap.error(f"--feature_type '{args.feature_type}' is not supported (only 'hubert')")
    if args.num_clusters < 1:
        ap.error("--num_clusters must be >= 1")
    if args.tol != 0.0:
        ap.error("--tol must be 0 (fairseq's setting); stopping on the centres' movement is not implemented")
    if args.reassignment_ratio != 0.0:
        ap.error("--reassignment_ratio must be 0 (fairseq's setting); random reassignment is not implemented")
    if args.init != "k-means++":
        ap.error("--init must be 'k-means++'")
    if not 0.0 < args.sample_pct <= 1.0:
        ap.error("--sample_pct must be in (0, 1]")
    if args.features_path is None:
        if not (args.checkpoint_path and args.manifest_path and args.layer is not None):
            ap.error("--checkpoint_path, --layer and --manifest_path are required without --features_path")
        if not os.path.isdir(args.checkpoint_path):
            ap.error(f"--checkpoint_path '{args.checkpoint_path}' is not a directory: an HF model directory is expected; "
                     "fairseq's .pt checkpoint format is out of scope (convert it to the HF layout first)")
    import numpy as np
    import torch
    U = importlib.import_module("multimodal-s2ut_amd.units")
    KM = importlib.import_module("multimodal-s2ut_amd.kmeans")
    if args.features_path is not None:
        feats = torch.from_numpy(np.load(args.features_path).astype(np.float16)).to(args.device).contiguous()
    else:
        model = U.HubertUnits.from_pretrained(args.checkpoint_path, None, args.layer, args.device)
        feats = KM.sample_features(model, args.manifest_path, args.sample_pct, args.seed, args.extension)
    if args.out_features_path:
        np.save(args.out_features_path, feats.cpu().numpy())
    km, secs = KM.learn_kmeans(feats, args.num_clusters, max_iter=args.max_iter, batch_size=args.batch_size,
                               max_no_improvement=args.max_no_improvement, n_init=args.n_init, seed=args.seed)
    KM.save_centroids(args.out_kmeans_model_path, km)
    print(f"frames {feats.shape[0]}, steps {km.n_steps_}, EWA inertia {km.ewa_inertia_:.6f}, fit {secs:.3f} s; "
          f"wrote {args.out_kmeans_model_path}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
