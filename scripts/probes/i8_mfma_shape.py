"""The two int8 MFMA shapes from registers on ONE device: v_mfma_i32_32x32x32_i8 against v_mfma_i32_16x16x64_i8
(ops.probe_mfma_i8_shape), alternating in one process after >= 2 s of back-to-back launches on random operands, at one and
at two waves per SIMD.  The decision figure is the random-operand ratio 16 / 32 set against the probe's own spread (max - min
over the repetitions).   python scripts/probes/i8_mfma_shape.py [reps] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from modegpt_amd import ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None

t0 = time.time()
while time.time() - t0 < 2.5:  # the clock settles under load
    ops.probe_mfma_i8_shape(32, random_operands=True, waves_per_simd=2)
    ops.probe_mfma_i8_shape(16, random_operands=True, waves_per_simd=2)

res = {"device": torch.cuda.get_device_name(0), "iters": 200000, "reps": reps, "unit": "TOP/s", "rates": {}}
for waves in (1, 2):
    for random in (True, False):
        runs = {32: [], 16: []}
        for _ in range(reps):
            for shape in (32, 16):  # alternating
                runs[shape].append(round(ops.probe_mfma_i8_shape(shape, random_operands=random, waves_per_simd=waves), 1))
        key = "%d_wave_per_simd_%s" % (waves, "random" if random else "zero")
        entry = {}
        for shape in (32, 16):
            r = runs[shape]
            entry["shape_%d" % shape] = {"runs": r, "mean": round(sum(r) / len(r), 1), "min": min(r), "max": max(r),
                                         "spread": round(max(r) - min(r), 1)}
        entry["ratio_16_over_32_of_means"] = round(entry["shape_16"]["mean"] / entry["shape_32"]["mean"], 4)
        entry["gap_16_minus_32_of_means"] = round(entry["shape_16"]["mean"] - entry["shape_32"]["mean"], 1)
        res["rates"][key] = entry
        print(key, json.dumps(entry), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
