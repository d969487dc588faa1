#!/usr/bin/env python3
"""Writes tests/golden/dropin_reference.json for tests/test_dropin_cpu.py: what the reference's builder text
(predict_model/*.py of the reference tree) produces on building_detection_amd.tfshim - parameter shapes and kinds,
output shape, FLOPs, node census and BatchNorm+ReLU fusions of each of the five models.  Data only; no reference
source is stored.

    python tests/golden/make_dropin.py PATH/TO/REFERENCE/predict_model"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_dropin_cpu as D  # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    if not D.reference_readable(ref):
        raise SystemExit(f"{ref}: not a readable predict_model directory of the reference")
    rec = {name: D.summarise(D.build_reference(name, ref)) for name in D.CASES}
    with open(D.GOLDEN, "w", encoding="utf-8") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {D.GOLDEN} ({os.path.getsize(D.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
