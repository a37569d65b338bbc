#!/usr/bin/env python3
"""Generate tests/golden/reference_pipelines.json: the `train_pipeline` and `test_pipeline` of the reference's config files
evaluated by `Config.fromfile`, stored as values only (per config: the path it came from and the two pipelines; tuples as
{"__tuple__": [...]}, the encoding of reference_configs.json).  tests/test_augment.py builds every transform of them through
the PIPELINES registry, so the check runs without the reference tree.  No reference source is copied: the config files are
executed where they lie.

usage:  python tests/golden/make_pipeline_fixture.py --ref REFERENCE_CHECKOUT
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dump_model_cfgs import CONFIGS, plain  # noqa: E402
from srfdet3d_amd.compat.config import Config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of a checkout of the reference")
    a = ap.parse_args()
    out = {}
    for name, rel in CONFIGS.items():
        cfg = Config.fromfile(os.path.join(a.ref, rel))
        out[name] = dict(source=rel, train_pipeline=plain(cfg.train_pipeline), test_pipeline=plain(cfg.test_pipeline))
    with open(os.path.join(HERE, "reference_pipelines.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "configs")


if __name__ == "__main__":
    main()
