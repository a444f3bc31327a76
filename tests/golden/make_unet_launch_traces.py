"""Records tests/golden/unet_launch_traces.json and prints the pack hashes of tests/test_unet_launches_host.py.

Run on the commit whose behaviour is the reference (the traces in the repository come from the last commit before the U-Net walk,
the conv packs and the profiling bracket of hip/drunet.py were single-sourced; the cases from `infer2d_wino4` on from the last
commit that kept the tail-split policy in `DRUNet._tail_split`, where `infer2d_wino4_lane` was recorded with that attribute set to
False around the call); needs the built library, no GPU:

    python tests/golden/make_unet_launch_traces.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_unet_launches_host as T  # noqa: E402

traces = {case: T.trace(case) for case in T.CASES}
for case, launches in traces.items():
    print(f"{case}: {len(launches)} launches")
assert any(name == "dinv_conv3x3_winograd4" for name, _ in traces["infer2d_wino4"]), "infer2d_wino4 misses the F(4x4) kernel"
with open(T.GOLDEN, "w") as f:
    f.write("{\n" + ",\n".join(f'"{case}": ' + json.dumps(l, separators=(",", ":")) for case, l in traces.items()) + "\n}\n")
for name in T.PACKS:
    print(f'    "{name}": {T.pack_hash(name)}')
