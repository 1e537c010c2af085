"""One rank of a world-2 validation pass (gloo process group) — launched by
tests/test_gpu_validate_dp.py as a fresh child process (test infrastructure).

    RANK=r LOCAL_RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p MMS2UT_DIST_BACKEND=gloo \
        python tests/validate_dp_child.py OUT_DIR

Each rank validates its share ``batches[rank::world]`` of the five-batch split (3 and 2 batches:
unequal counts, the pass's only collective is its final all-reduce) and writes the stats it got to
OUT_DIR/rank{r}.json.
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from oracle import ref_model as R  # noqa: E402

mm = importlib.import_module("multimodal-s2ut_amd")

SHAPES = (([120, 90], [30, 22]), ([100, 77, 60], [25, 20, 15]), ([61, 47, 30], [14, 11, 9]), ([53, 40], [12, 8]),
          ([88], [19]))


def model_cfg():
    return mm.default_cfg(**R.tiny_config(conv_channels=256))      # dropout 0.1: eval mode must ignore it


def validate(rank, world):
    cfg = model_cfg()
    model = mm.MMS2UTModel(cfg, device="cuda").init_params(seed=5)
    tr = mm.trainer.Trainer(model, lr=1e-3, world_size=world)
    samples = [mm.data.make_sample(L, T, img_tokens=17, img_dim=cfg["image_feat_dim"], seed=s)
               for s, (L, T) in enumerate(SHAPES)]
    mine = samples[rank::world]
    return tr.validate(mm.runtime.prepare_batch(s, cfg, "cuda") for s in mine)


def main(out_dir):
    rank, world, local = mm.parallel.init_from_env()
    torch.cuda.set_device(local)
    stats = validate(rank, world)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(stats, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
