"""Golden fixtures for the beam decode of speech units, written by running the reference's OWN code.

Loads ``mm_s2ut/scripts/speech_to_speech_translation/mhubert.py`` from the reference checkout (``torchaudio``,
``joblib`` and ``transformers`` stubbed in ``sys.modules``: ``decode`` uses none of them) and calls ``HubertCode.decode`` unbound on an object that carries ``C``, ``Cnorm`` and ``C_np``,
with ``beamsearch=True``.  Writes ``tests/golden/units_beam_<case>.npz``:

  features fp32 [T, d] (fp16-representable), centroids fp32 [Kc, d], top_k, beamsize,
  idx int32 / val fp32 [T, top_k] (the reference's torch.topk), code, beam_code, beam_merged_code,
  numpy (the NumPy version: under NumPy >= 2 the reference's scores are float32),
  ties: how many adjacent pairs of equal scores the kept beam held, summed over the frames, counted by
  replaying units.beam_steps on the reference's (idx, val).

The features are centroids plus noise, and a frame repeats the previous frame's centroid with probability
0.6, so that runs exist.  This script contains no reference source and never runs on a GPU machine: it
needs the reference checkout (``MMS2UT_REFERENCE``, default ``reference`` next to this repository) and skips
itself when that is absent.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_units_beam_golden.py
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MMS2UT_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden")
SOURCE = os.path.join(REF, "mm_s2ut", "scripts", "speech_to_speech_translation", "mhubert.py")

# name -> (T, Kc, d, top_k, beamsize, seed)
CASES = {
    "a": (12, 32, 16, 4, 8, 1),
    "b": (40, 100, 16, 10, 200, 2),
    "c": (25, 64, 8, 10, 200, 3),
    "one": (1, 16, 8, 1, 1, 4),          # one frame, greedy
    "open": (9, 16, 8, 3, 200, 5),       # every candidate is kept until 3^5 = 243 of them exceed the beam
}


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _load_reference():
    for name in ("torchaudio", "joblib", "transformers"):
        sys.modules[name] = _Stub(name)
    spec = importlib.util.spec_from_file_location("ref_mhubert", SOURCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)           # reference code, run from its checkout
    return mod


def _inputs(T, Kc, d, seed):
    r = np.random.default_rng(seed)
    cents = r.standard_normal((Kc, d)).astype(np.float32)
    which = np.empty(T, dtype=np.int64)
    for t in range(T):
        which[t] = which[t - 1] if t and r.random() < 0.6 else r.integers(Kc)
    feats = cents[which] + 0.35 * r.standard_normal((T, d)).astype(np.float32)
    return feats.astype(np.float16).astype(np.float32), cents


def main():
    if not os.path.isfile(SOURCE):
        print("reference absent; nothing to do")
        return 0
    sys.path.insert(0, ROOT)
    U = importlib.import_module("multimodal-s2ut_amd.units")
    ref = _load_reference()
    os.makedirs(OUT, exist_ok=True)
    total, any_ties, any_diff = 0, False, False
    for name, (T, Kc, d, top_k, beamsize, seed) in CASES.items():
        feats, cents = _inputs(T, Kc, d, seed)
        C_np = np.ascontiguousarray(cents.transpose())
        holder = types.SimpleNamespace(C_np=C_np, C=torch.from_numpy(C_np),
                                       Cnorm=torch.from_numpy(np.square(C_np).sum(0, keepdims=True)))
        feature = torch.from_numpy(feats)
        seen, topk = [], torch.topk
        torch.topk = lambda *a, **kw: seen.append(topk(*a, **kw)) or seen[-1]     # the top-k the beam runs on
        try:
            out = ref.HubertCode.decode(holder, feature, beamsearch=True, top_k=top_k, beamsize=beamsize)
        finally:
            torch.topk = topk
        top, = seen
        idx, val = top.indices.numpy().astype(np.int32), top.values.numpy().astype(np.float32)
        code = np.asarray(out["code"], dtype=np.int32)
        beam = np.asarray([int(u) for u in out["beam_code"]], dtype=np.int32)
        merged = np.asarray([int(u) for u in out["beam_merged_code"]], dtype=np.int32)
        assert np.array_equal(code, idx[:, 0]) and len(beam) == T and np.isfinite(val).all()
        ties = sum(int((sc[1:] == sc[:-1]).sum()) for _, _, sc in U.beam_steps(idx, val, beamsize))
        mine = U.beam_decode_host(idx, val, beamsize)
        any_ties |= ties > 0
        any_diff |= not np.array_equal(beam, code)
        path = os.path.join(OUT, f"units_beam_{name}.npz")
        np.savez_compressed(path, features=feats, centroids=cents, top_k=np.int64(top_k), beamsize=np.int64(beamsize),
                            idx=idx, val=val, code=code, beam_code=beam, beam_merged_code=merged,
                            numpy=np.array(np.__version__), ties=np.int64(ties))
        total += os.path.getsize(path)
        print(f"units_beam_{name}: T={T} Kc={Kc} d={d} top_k={top_k} beamsize={beamsize}: greedy {len(U.merge(code))} "
              f"merged units, beam {len(merged)}; ties in the kept beam {ties}; host restatement equal: "
              f"{mine == beam.tolist()} ({os.path.getsize(path)} B)")
    assert any_ties, "no case has score ties inside the kept beam"
    assert any_diff, "beam_code equals code in every case"
    assert int(np.__version__.split(".")[0]) >= 2, "the fixtures pin the float32 (NumPy >= 2) evaluation"
    assert total < 100 * 1024, f"fixtures too large: {total} B"
    return 0


if __name__ == "__main__":
    sys.exit(main())
