#!/usr/bin/env python
"""The UNet's inference forward and training step on the device against oracle/torch_port.py in float64, next to the float32
port's own error on the same case: one line per case and kernel form (tests/unet_f64_cases.py holds the cases, the forms and the
metrics; tests/test_hip_unet_f64.py asserts bounds chosen from this table).

    python tools/unet_f64_report.py > profiles/unet_f64.txt
    python tools/unet_f64_report.py --cases A B --forms default WINO=4

Columns: error of the device / of the float32 port / their ratio (the port's error floored at 2^-23), for the forward (worst
plane of any sample), the loss terms, the worst gradient tensor E_k (with its name) and the zero-gradient noise Z_k; for a forced form, how it showed that it ran.
A case whose width the training kernels do not take (U.CASES[..]["train_refused"]) has its forward columns and the library's
refusal of the step.  Then one fused sampler step per width (U.STEP_CASES; tests/test_hip_unet_widths.py): x_{t-1} and pred_xstart
of the DDPM and the DDIM update against float64, device / float32 port and oracle / ratio."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import unet_f64_cases as U  # noqa: E402


def _cell(dev, prt, rat, key):
    return f"{dev[key]:.2e} {prt[key]:.2e} {rat[key]:6.2f}" if key in dev else f"{'-':>8} {'-':>8} {'-':>6}"


def line(case, form, dev, prt):
    rat = U.ratios(dev, prt)
    return (f"{case:<5}{form:<18}| {_cell(dev, prt, rat, 'fwd')} | {_cell(dev, prt, rat, 'loss')} | {_cell(dev, prt, rat, 'grad')} "
            f"{dev.get('grad_name', '-'):<48} | {_cell(dev, prt, rat, 'zero')}" + (f" | {dev['ran']}" if "ran" in dev else ""))


_default_forward = {}


def run(case, name, value, forward, training, autograd=False):
    """device_errors of one (case, form), with "ran": how a forced form showed that it ran (tests/unet_f64_cases.py)."""
    form, kernels = f"{name}={value}", {} if name else None
    with U.forced(name, value):
        y = U.device_forward(case, kernels) if forward else None
        step = U.device_step(case, autograd=autograd, kernels=kernels) if training else None
    dev = U.device_errors(case, y, step)
    if name is None:
        _default_forward[case] = y if y is not None else _default_forward.get(case)
        return dev
    rule = (U.FORWARD_ENGAGED if forward else U.TRAINING_ENGAGED).get(form)
    if rule:
        dev["ran"] = U.engaged(kernels, rule) or f"ran {rule[1]}"
    elif forward and case in U.FORWARD_DIFFERS.get(form, ()):
        dev["ran"] = "bits differ from the default's" if not (y == _default_forward[case]).all() else "NOT ENGAGED: the default's bits"
    return dev


def refusal(case):
    """What the library answers to a case it must refuse."""
    try:
        U.device_forward(case)
    except NotImplementedError as e:
        assert U.CASES[case]["refused"] in str(e), e
        return f"refused: {e}"
    raise AssertionError(f"case {case} ran; the library should refuse it ({U.CASES[case]['refused']})")


def train_refusal(case):
    """What the library answers to a training step at a width it does not train."""
    try:
        U.device_step(case)
    except NotImplementedError as e:
        assert U.CASES[case]["train_refused"] in str(e), e
        return f"step refused: {e}"
    raise AssertionError(f"case {case} trained; the library should refuse the step ({U.CASES[case]['train_refused']})")


def step_lines(cases):
    print("# one fused sampler step  | x_{t-1}: device port32 ratio, where            | pred_xstart: device port32 ratio, where")
    worst = (0.0, "")
    for case in cases:
        for mode in U.STEP_MODES:
            dev = U.step_errors(case, mode, *U.device_fused_step(case, mode))
            prt = U.step_errors(case, mode, *U.step_reference(case)[mode]["f32"])
            cells = []
            for d, p in zip(dev, prt):
                r = d[0] / max(p[0], U.EPS32)
                worst = max(worst, (r, f"{case} {mode}"))
                cells.append(f"{d[0]:.2e} {p[0]:.2e} {r:6.2f} {str(d[1]):<14}")
            print(f"{case:<5}{mode:<18}| " + " | ".join(cells), flush=True)
    print(f"# worst ratio, fused step: {worst[0]:.2f} ({worst[1]})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=list(U.CASES))
    ap.add_argument("--forms", nargs="*", default=None, help="default, autograd, step (the fused sampler step) or NAME=VALUE; all of them when not given")
    a = ap.parse_args()
    print(f"# {'case form':<21}| forward: device port32 ratio | loss: device port32 ratio   | worst E_k: device port32 ratio, tensor"
          f"{'':<43} | Z_k: device port32 ratio")
    worst = {}
    for case in a.cases:
        prt = U.port_errors(case)
        jobs = [("default", None, None, True, True, False)]
        if U.CASES[case]["w"] is not None:
            jobs.append(("autograd", None, None, False, True, True))
        jobs += [(f"{n}={v}", n, v, True, False, False) for n, v in U.FORWARD_FORMS if case in U.FORWARD_FORM_CASES]
        jobs += [(f"{n}={v} step", n, v, False, True, False) for n, v in U.TRAINING_FORMS if case in U.TRAINING_FORM_CASES]
        for form, n, v, fwd, trn, ag in jobs:
            if a.forms is not None and form.split()[0] not in a.forms:
                continue
            if U.CASES[case]["refused"]:
                print(f"{case:<5}{form:<18}| {refusal(case)}", flush=True)
                continue
            refused = U.CASES[case]["train_refused"] and trn
            dev = run(case, n, v, fwd, trn and not refused, ag)
            print(line(case, form, dev, prt) + (f" | {train_refusal(case)}" if refused else ""), flush=True)
            kind = "default forms" if n is None else "forced forms"
            for k, r in U.ratios(dev, prt).items():
                worst[kind, k] = max(worst.get((kind, k), (0.0, "")), (r, f"{case} {form}"))
    for (kind, k), (r, where) in sorted(worst.items()):
        print(f"# worst ratio, {kind}, {k}: {r:.2f} ({where})")
    if a.forms is None or "step" in a.forms:
        step_lines([c for c in U.STEP_CASES if c in a.cases])


if __name__ == "__main__":
    main()
