"""numpy fp64 restatement of one item of the Tianchi per-beat dataset with every draw given: what nef_beat_batch and the plan of
dataset/resident.py must reproduce bit for bit.  tests/test_resident_cpu.py anchors it to EcgTianChiInterval.__getitem__ itself.

Also the small fixtures the resident tests share: the bundled recordings, a cfg on a label list of them, synthetic stores."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "tianchi")
NAMES = ("11315", "40723")
KEYS = ("P on", "P off", "R on", "R off", "T on", "T off")
L = 512
# (lead_num, super_mode, train_data_mode): the random 3-lead mode and the fixed schemes of 1, 2, 8 and 12 input leads
SCHEMES = ((3, "normal", "normal"), (1, "_192", "normal"), (2, "_228", "normal"), (8, "_8120", "normal"), (12, "_12120", "normal"))


def lead_theta():
    from electrocardio_panorama_amd.synth import LEAD_THETA
    return LEAD_THETA


def _fit(a):
    out = np.zeros(a.shape[:-1] + (L,), dtype=a.dtype)
    m = min(L, a.shape[-1])
    out[..., :m] = a[..., :m]
    return out


def beat_item(signal8, labels, beat, sel, target, rest, theta=None):
    """signal8 [8, len] (any real dtype), labels {key: list}, the drawn beat, input leads, target lead and rest leads -> the item's fields."""
    theta = lead_theta() if theta is None else theta
    s = np.asarray(signal8).astype(np.float64)
    i, ii = s[0:1], s[1:2]
    s = np.concatenate([s, ii - i, -0.5 * (i + ii), i - 0.5 * ii, ii - 0.5 * i], axis=0)
    p_on, p_off, r_on, r_off, t_on, t_off = (int(labels[k][beat]) for k in KEYS)
    end = int(labels["P on"][beat + 1])
    rois = np.array([[p_on, p_off], [p_off, r_on], [r_on, r_off], [r_off, t_on], [t_on, t_off], [t_off, end], [end, L + p_on]]) - p_on
    s = s[:, p_on:end]
    lo, hi = np.min(s), np.max(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (s - lo) / (hi - lo)
    sel, rest = list(sel), list(rest)
    return {"data": _fit(s[sel]).astype(np.float32), "rois": rois.astype(np.int64), "input_theta": theta[sel].astype(np.float32),
            "target_view": _fit(s[target]).astype(np.float32), "target_theta": theta[target].astype(np.float32),
            "rest_view": _fit(s[rest]).astype(np.float32).reshape(len(rest), L), "rest_theta": theta[rest].astype(np.float32).reshape(len(rest), 2)}


def recordings():
    """[(name, signal [8, 5000] int16, {key: list})] of the two bundled recordings."""
    out = []
    for n in NAMES:
        z = np.load(os.path.join(GOLD, n + ".npz"))
        out.append((n + ".json", z["signal"], {k: z[k.replace(" ", "_")].tolist() for k in KEYS}))
    return out


def make_cfg(listing, scheme=SCHEMES[0], data_root=GOLD, label_root=GOLD):
    from electrocardio_panorama_amd.config import get_defaults, resolve_config_path
    cfg = get_defaults()
    cfg.merge_from_file(resolve_config_path("config/nef_net.yml"))
    cfg.DATA.dataset = "tianchi"
    cfg.DATA.test_label_path = cfg.DATA.train_label_path = str(listing)
    cfg.DATA.train_data_root, cfg.DATA.train_label_root = str(data_root), str(label_root)
    cfg.DATA.lead_num, cfg.DATA.super_mode, cfg.DATA.train_data_mode = scheme
    cfg.MODEL.jitter_factor = 0.0
    return cfg


def write_listing(tmp_path, names=tuple(n + ".json" for n in NAMES), repeat=1):
    p = tmp_path / "jsons.txt"
    p.write_text("\n".join(list(names) * repeat) + "\n")
    return p


def write_tree(tmp_path, recs):
    """recs: [(stem, signal [8, len], {key: list})] -> a .npy + .json tree and its label list; returns the listing."""
    os.makedirs(tmp_path / "npy", exist_ok=True)
    os.makedirs(tmp_path / "json", exist_ok=True)
    import json
    for stem, sig, lab in recs:
        np.save(tmp_path / "npy" / (stem + ".npy"), sig)
        (tmp_path / "json" / (stem + ".json")).write_text(json.dumps({k: [int(v) for v in lab[k]] for k in KEYS}))
    p = tmp_path / "list.txt"
    p.write_text("\n".join(stem + ".json" for stem, _, _ in recs) + "\n")
    return p


def labels_for(p_ons):
    """Plausible marks inside every beat of the given P onsets (the last entry only ends the last beat)."""
    p = np.asarray(p_ons, dtype=np.int64)
    n = np.diff(p)
    inner = lambda f: (p[:-1] + (n * f).astype(np.int64)).tolist() + [int(p[-1])]      # noqa: E731
    return {"P on": p.tolist(), "P off": inner(0.15), "R on": inner(0.25), "R off": inner(0.4), "T on": inner(0.6), "T off": inner(0.8)}


def plan_items(store, plan, signals=None):
    """The restatement's items for every row of a Plan of dataset/resident.py, stacked like a collated batch."""
    sig = store.signal.cpu().numpy()
    items = []
    for j, name in enumerate(plan.id):
        i = store.names.index(name)
        s8 = sig[store.offsets[i]:store.offsets[i + 1]].reshape(8, -1)
        lab = {k: store.labels[q][store.label_offsets[q][i]:store.label_offsets[q][i + 1]].tolist() for q, k in enumerate(KEYS)}
        row = plan.table[j, 3:].tolist()
        items.append(beat_item(s8, lab, int(plan.beats[j]), row[:plan.V], row[plan.V], row[plan.V + 1:]))
    return {k: np.stack([it[k] for it in items]) for k in items[0]}
