#!/usr/bin/env python3
"""Share of the per-trajectory controller kernels in a rollout's GPU time, from a rocprofv3 --kernel-trace database:
    rocprofv3 --kernel-trace --stats -d OUT -o traj -- python tools/traj_dopri_bench.py --B 65536 --modes trajectory
    python tools/traj_prof_share.py OUT/traj_results.db
Prints the kernel-time table (total ms, launches) and the controller share: traj_*_kernel (stage inputs and stage times,
error ratio / decisions / dense output, initial step) plus the dlogp / reverse-time scale kernel over all kernel time."""
import sqlite3
import sys
from collections import defaultdict


def main(path):
    c = sqlite3.connect(path)
    tot, cnt = defaultdict(float), defaultdict(int)
    for name, dur in c.execute("select name, duration from kernels"):
        short = name.split("(")[0].replace("void ", "")
        tot[short] += dur * 1e-6
        cnt[short] += 1
    all_ms = sum(tot.values())
    ctl = sum(v for k, v in tot.items() if "traj_" in k)
    for k, v in sorted(tot.items(), key=lambda kv: -kv[1]):
        print(f"{v:12.3f} ms {cnt[k]:7d}  {100 * v / all_ms:6.2f} %  {k[:110]}")
    print(f"controller + dense-output kernels (traj_*): {ctl:.3f} ms of {all_ms:.3f} ms = {100 * ctl / all_ms:.3f} %")


if __name__ == "__main__":
    main(sys.argv[1])
