"""mms2ut-wer: the reference's mm_s2ut/scripts/wer.py on the HIP edit-distance kernel (see wer_cli.py):
reference text + transcripts, paired by line -> WER, errors, reference words."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    sys.exit(importlib.import_module("multimodal-s2ut_amd.wer_cli").main())
