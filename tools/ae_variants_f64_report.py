#!/usr/bin/env python
"""The auto-encoder training step of the geometry-only, skip and PBR networks against float64 autograd, case by case
(tests/ae_f64_cases.py holds the cases, the batches and the metrics; tests/test_hip_ae_variants_f64.py asserts the bounds).

    python tools/ae_variants_f64_report.py > profiles/ae_variants_f64.txt
    python tools/ae_variants_f64_report.py --cases pbr-3x3x3-N63-cell
    python tools/ae_variants_f64_report.py --gaps          # the BOUNDS table of tests/ae_f64_cases.py, from the CPU alone

Per case and quantity: the bound, the float32 restatement's own error against float64 (the gap the bound comes from, measured
here on the CPU) and, where a GPU is present, the device's error — what the test hands to record_property.  For the gradients
the worst tensor is named.  Without a GPU the device columns are left out and the table says so."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import ae_f64_cases as A  # noqa: E402


def gaps_table(cases):
    print("BOUNDS = {")
    for case in cases:
        gap = A.float32_gap(case)
        cells = [f"({A.bound_for(q, gap[q]):.1e}, {gap[q]:.2e})" for q in A.quantities(case)]
        print(f'    "{case}":\n        _row(' + ",\n             ".join(", ".join(cells[i:i + 3]) for i in range(0, len(cells), 3)) + "),")
    print("}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=list(A.CASES))
    ap.add_argument("--gaps", action="store_true")
    a = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if a.gaps:
        return gaps_table(a.cases)
    gpu = torch.cuda.is_available()
    print("# auto-encoder variants against float64: bound / float32 restatement (CPU) / device" if gpu else
          "# auto-encoder variants against float64: bound / float32 restatement (CPU); no GPU here, so no device column")
    for case in a.cases:
        c = A.CASES[case]
        gap = A.float32_gap(case)
        dev = None
        if gpu:
            net, _ = A.network(case)
            dev = A.device_run(case, net)
        pts, sdf, _ = A.batch(case)
        rows = int((sdf[:, 0].abs().numpy() < A.band(case)).sum())
        print(f"{case}: planes {'x'.join(map(str, c['hwd']))} config {c['cfg']} tex_channels {c['tc']} N {c['N']} {c['place']} "
              f"band rows {rows} kink distance {A.kink_distance(case):.1e}")
        for q in A.quantities(case):
            line = f"    {q:<7} bound {A.BOUNDS[case][q][0]:.1e}  float32 {gap[q]:.2e}"
            if dev is not None:
                line += f"  device {dev[q]:.2e}"
            if q == "grad":
                line += f"  worst tensor {gap['grad_at']}" + (f" / {dev['grad_at']}" if dev is not None else "")
            print(line)
        if dev is not None:
            print(f"    decode  bound {A.BOUNDS[case]['pred'][0]:.1e}  device " +
                  (f"{dev['decode']:.2e}" if dev["decode"] is not None else "refused: no compiled inference decoder for these widths"))
            print(f"    losses  {' '.join(f'{v:.6g}' for v in dev['losses'])}  same bits again: {dev['again_same']}", flush=True)


if __name__ == "__main__":
    main()
