#!/usr/bin/env python
"""The decode path on the device against the restatement tests/pbr_cases.py in float64, next to the float32 restatement's own
error on the same case: one line per case and stage (tests/decoder_f64_cases.py holds the cases, the points and the metrics;
tests/test_hip_decoder_f64.py asserts bounds chosen from this table).

    python tools/decoder_f64_report.py > profiles/decoder_f64.txt
    python tools/decoder_f64_report.py --cases A H

Columns: error of the device / of the float32 restatement / their ratio (the restatement's error floored at 2^-23); for the
plane stage the worst (group, plane), for the point stage the worst column and where its worst point sits in the launch, for
grid mode the worst column and cell and the agreement of grid mode with point mode on the same centres.  Then, per case, how
many points (all / designed rows) meet each border condition on each plane's row and column coordinate, and the K's the
ratios give: twice the worst ratio, rounded up to a power of two."""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import decoder_f64_cases as Dc  # noqa: E402


def _place(p):
    return (f"point {p['point']} (block {p['block']}, wave {p['wave']}, lane {p['lane']}, half {p['half']}, "
            f"{'designed' if p['designed'] else 'uniform'})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=list(Dc.CASES))
    a = ap.parse_args()
    print(f"# {'case net   up/hid  kernel':<40}| stage | device   float32  ratio | where")
    worst = {}
    for case in a.cases:
        c = Dc.CASES[case]
        yard = Dc.yardstick(case)
        over = {k: yard[k] for k, cap in Dc.CAPS.items() if k in yard and yard[k] > cap}
        assert not over, f"reference ill-conditioned: choose other inputs ({case}: {over})"
        dev = Dc.device_errors(case, Dc.device_run(case))
        rat = Dc.ratios(dev, yard)
        head = f"{case:<5}{c['kind']:<6}{c['up']:>3}/{c['hid']:<4}k_decode{c['kernel']:<22}"
        where = {"plane": "%s %s" % dev["plane_at"], "point": f"column {dev['point_col']}, {_place(dev['point_place'])}"}
        if "grid" in dev:
            where["grid"] = (f"column {dev['grid_col']}, cell {dev['grid_cell']} of {'x'.join(map(str, Dc.GRID_DIMS[case]))}; "
                             f"grid mode vs point mode {dev['grid_vs_points']:.2e}")
        where["sdf"] = "column 0 against its own float32 error"
        for stage in ("plane", "point", "sdf", "grid"):
            if stage in dev:
                print(f"{head:<42}| {stage:<5} | {dev[stage]:.2e} {yard[stage]:.2e} {rat[stage]:5.2f} | {where[stage]}", flush=True)
                worst[stage] = max(worst.get(stage, (0.0, "")), (rat[stage], case))
        n = max(c["n"])
        cond = Dc.input_conditions(case, n)
        cells = [f"{p}.{w} " + " ".join(f"{k} {v[0]}/{v[1]}" for k, v in cond[p, w].items()) for p, w in cond]
        print(f"#     {n} points, {len(Dc.designed_rows(n))} designed rows {Dc.designed_rows(n)}; clamped low / high / at a texel "
              f"centre, all/designed: " + "; ".join(cells))
    for stage, (r, case) in worst.items():
        k = 2 ** max(0, math.ceil(math.log2(2 * r)))
        print(f"# worst ratio, {stage}: {r:.2f} (case {case}) -> K_{stage.upper()} = {k}")


if __name__ == "__main__":
    main()
