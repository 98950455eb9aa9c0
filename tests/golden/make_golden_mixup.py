"""Generate tests/golden/mixup.pt by running the UNMODIFIED reference Mixup (lib/datasets/mixup.py: numpy + torch only).

Run where a reference checkout is available (PVRL_REFERENCE_DIR, default ../reference next to this repository):
    python tests/golden/make_golden_mixup.py
The module is loaded from its file as it is; nothing of its source is copied, only inputs and outputs are stored.  The draws
are recorded by wrapping, on the loaded module and on each Mixup instance, the functions the reference calls
(`_params_per_batch` / `_params_per_elem`, `cutmix_bbox_and_lam`, `mixup_target`): their arguments and results are kept,
their behaviour is untouched.

Per case (Mixup keyword arguments + np.random seed) a few consecutive calls on one Mixup object are recorded:
  params   the (lam, use_cutmix) the call drew, before any correction
  boxes    [(yl, yh, xl, xh), corrected lam] of every cut, in draw order
  lam      the lam the reference hands mixup_target (float, or a per-clip fp32 vector)
and, for the first calls of the cases in OUT_CASES, the mixed batch and the dense targets (int labels; EPIC verb / noun dict).
Inputs are NOT stored: x = torch.randn(SHAPE) after torch.manual_seed(X_SEED + call).  SHAPE has T < H < W so that both the
frame (T) and the row (H) clamp of the cut box are exercised.
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PVRL_REFERENCE_DIR", os.path.join(ROOT, "..", "reference"))
sys.dont_write_bytecode = True

SHAPE = (4, 3, 4, 8, 12)
X_SEED = 1234
NUM_CLASSES = 10
SMOOTHING = 0.1
EK = dict(mixup_alpha=0.1, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)     # configs/EK/egocentric_action_classification.yaml
CASES = [
    ("batch_ek", dict(EK, mode="batch"), 3, 6),
    ("batch_minmax", dict(EK, mode="batch", cutmix_minmax=[0.2, 0.8]), 5, 4),
    ("batch_prob", dict(EK, mode="batch", prob=0.5), 11, 4),
    ("batch_switch0", dict(EK, mode="batch", switch_prob=0.0), 7, 2),
    ("batch_switch1", dict(EK, mode="batch", switch_prob=1.0), 8, 3),
    ("batch_nocorrect", dict(EK, mode="batch", switch_prob=1.0, correct_lam=False), 9, 2),
    ("batch_cutmix_only", dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="batch"), 10, 2),
    ("pair_ek", dict(EK, mode="pair"), 21, 4),
    ("pair_minmax", dict(EK, mode="pair", cutmix_minmax=[0.3, 0.9]), 22, 3),
    ("elem_ek", dict(EK, mode="elem"), 31, 4),
    ("elem_minmax", dict(EK, mode="elem", cutmix_minmax=[0.2, 0.8]), 32, 3),
    ("elem_prob", dict(EK, mode="elem", prob=0.5, switch_prob=1.0), 33, 3),
    ("elem_mixup_only", dict(mixup_alpha=0.4, cutmix_alpha=0.0, mode="elem"), 34, 2),
]
OUT_CASES = {"batch_ek": 3, "batch_minmax": 3, "batch_prob": 3, "pair_ek": 1, "pair_minmax": 2, "elem_ek": 2, "elem_minmax": 1,
             "elem_prob": 1}


def load_reference_mixup():
    spec = importlib.util.spec_from_file_location("ref_mixup", os.path.join(REF, "lib", "datasets", "mixup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(v):
    return torch.as_tensor(np.asarray(v)).clone()


def record_case(ref, kwargs, seed, calls, n_out):
    rec = {"boxes": [], "lam_in": None}
    orig_box, orig_target = ref.cutmix_bbox_and_lam, ref.mixup_target

    def box(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
        (yl, yh, xl, xh), lam2 = orig_box(img_shape, lam, ratio_minmax=ratio_minmax, correct_lam=correct_lam, count=count)
        rec["boxes"].append(([int(yl), int(yh), int(xl), int(xh)], float(lam2)))
        return (yl, yh, xl, xh), lam2

    def target(t, num_classes, lam=1., smoothing=0.0, device="cuda"):
        rec["lam_in"] = lam.clone() if torch.is_tensor(lam) else float(lam)
        return orig_target(t, num_classes, lam, smoothing, device)

    ref.cutmix_bbox_and_lam, ref.mixup_target = box, target
    try:
        m = ref.Mixup(label_smoothing=SMOOTHING, num_classes=NUM_CLASSES, **kwargs)
        for name in ("_params_per_batch", "_params_per_elem"):
            fn = getattr(m, name)

            def wrapped(*a, _fn=fn, **k):
                out = _fn(*a, **k)
                rec["params"] = copy.deepcopy(out)
                return out
            setattr(m, name, wrapped)
        np.random.seed(seed)
        out = []
        for c in range(calls):
            rec["boxes"], rec["params"], rec["lam_in"] = [], None, None
            torch.manual_seed(X_SEED + c)
            x = torch.randn(SHAPE)
            g = torch.Generator().manual_seed(X_SEED + 100 + c)
            labels = torch.randint(0, NUM_CLASSES, (SHAPE[0],), generator=g)
            epic = {"verb": torch.randint(0, 97, (SHAPE[0],), generator=g), "noun": torch.randint(0, 300, (SHAPE[0],), generator=g)}
            mixed, tgt = m(x, labels)
            lam_p, cut_p = rec["params"]
            call = {"params_lam": _np(lam_p).double(), "params_cutmix": _np(cut_p).bool(), "boxes": rec["boxes"],
                    "lam": rec["lam_in"], "labels": labels, "epic_labels": epic}
            if c < n_out:
                call["out"] = mixed.clone()
                call["target"] = tgt.clone()
                call["epic_target"] = orig_target(epic, NUM_CLASSES, rec["lam_in"], SMOOTHING, "cpu")
            out.append(call)
        return out
    finally:
        ref.cutmix_bbox_and_lam, ref.mixup_target = orig_box, orig_target


def main():
    ref = load_reference_mixup()
    fx = {"shape": SHAPE, "x_seed": X_SEED, "num_classes": NUM_CLASSES, "smoothing": SMOOTHING, "cases": {}}
    for name, kwargs, seed, calls in CASES:
        fx["cases"][name] = {"kwargs": kwargs, "seed": seed,
                             "calls": record_case(ref, kwargs, seed, calls, OUT_CASES.get(name, 0))}
    path = os.path.join(HERE, "mixup.pt")
    torch.save(fx, path)
    kinds = {n: [("cut" if c["boxes"] else "none" if (np.asarray(c["params_lam"]) == 1).all() else "blend") for c in v["calls"]]
             for n, v in fx["cases"].items()}
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for n, k in kinds.items():
        print(f"  {n}: {k}")


if __name__ == "__main__":
    main()
