#!/usr/bin/env python3
"""The first timed block of `bench.py` in a `rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -o run` directory:
every kernel dispatch and every HIP API call longer than --min-api-ms, from the last untimed step-train launch to the end of the
second timed launch, in ms from the start of that last untimed launch.  Prints one JSON object.

    tools/first_launch_trace.py <rocprofv3 output dir> [--untimed 4] [--min-api-ms 0.2]

--untimed: step-train launches before the timed ones (the plain run's settle 60 + warm-up 5 at 50 steps per call: 50, 10, 5 = 3;
the kernel name matches rem2d_step_train).  The excerpt ends with the second timed launch."""
import argparse
import csv
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--untimed", type=int, default=3)
    ap.add_argument("--min-api-ms", type=float, default=0.2)
    a = ap.parse_args()
    ks = list(csv.DictReader(open(os.path.join(a.dir, "run_kernel_trace.csv"))))
    api = list(csv.DictReader(open(os.path.join(a.dir, "run_hip_api_trace.csv"))))
    train = sorted((k for k in ks if "rem2d_step_train" in k["Kernel_Name"]), key=lambda k: int(k["Start_Timestamp"]))
    t0 = int(train[a.untimed - 1]["Start_Timestamp"])
    t1 = int(train[a.untimed + 1]["End_Timestamp"])
    ev = []
    for k in ks:
        s, e = int(k["Start_Timestamp"]), int(k["End_Timestamp"])
        if t0 <= s <= t1:
            ev.append({"t_ms": round((s - t0) / 1e6, 3), "dur_ms": round((e - s) / 1e6, 3), "kind": "kernel",
                       "name": k["Kernel_Name"].split("(")[0][:90], "grid": int(k["Grid_Size_X"])})
    for c in api:
        s, e = int(c["Start_Timestamp"]), int(c["End_Timestamp"])
        if t0 <= s <= t1 and (e - s) / 1e6 >= a.min_api_ms:
            ev.append({"t_ms": round((s - t0) / 1e6, 3), "dur_ms": round((e - s) / 1e6, 3), "kind": "hip_api", "name": c["Function"]})
    ev.sort(key=lambda d: d["t_ms"])
    durs = [round((int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e6, 3) for k in train]
    print(json.dumps({"source": a.dir, "step_train_launches_ms": durs, "untimed_launches": a.untimed,
                      "first_timed_launch_ms": durs[a.untimed], "events": ev}, indent=1))


if __name__ == "__main__":
    main()
