"""mms2ut-generate: the reference's fairseq-generate command line on the HIP path (see generate_cli.py):
checkpoint + manifest split -> generate-{subset}.txt and generate-{subset}.unit."""
import importlib
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, stream=sys.stderr, format="%(asctime)s | %(levelname)s | %(message)s")
    sys.exit(importlib.import_module("multimodal-s2ut_amd.generate_cli").main())
