"""Merge the records of scripts/feed_rate.py runs on JPEG frames into one table (profiles/jpeg_device_feed_rate.json).
    python scripts/merge_feed_rate.py DIR OUT [--note TEXT ...]
DIR holds <row>.<leg>.json files, written by `feed_rate.py --frames-dir ... --out DIR/<row>.<leg>.json`; legs: parent_host (the host route in
a checkout of the parent commit), new_host (the host route in this tree), new_device (--jpeg device), and optional repeats of the two host
legs named parent_host_2, new_host_2, ...  Every leg's record is kept verbatim under "legs"; per row this adds
    predicted_device_fps     = host-route rate x (whole-decode ms / coefficient-only ms), both single-thread times of the new_host run
    achieved_over_predicted  = device-route rate / predicted_device_fps
    device_over_host         = device-route rate / host-route rate (the gate: >= 1 on every row)
    host_new_over_parent     = every new_host* rate / every parent_host* rate, smallest and largest (the refactoring must not cost the host route)
"""
import glob
import json
import os
import sys


def main():
    d, out = sys.argv[1], sys.argv[2]
    notes = [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--note"]
    rows = {}
    for f in sorted(glob.glob(os.path.join(d, "*.json"))):
        row, leg = os.path.basename(f)[:-5].rsplit(".", 1)
        rows.setdefault(row, {})[leg] = json.load(open(f))
    table = []
    key = "feeder_fps_decode_upload_resize"
    for row, legs in rows.items():
        h, dv = legs["new_host"], legs["new_device"]
        pred = h[key] * h["decode_ms_per_frame_1_thread"] / h["coefficients_ms_per_frame_1_thread"]
        new = [v[key] for k, v in legs.items() if k.startswith("new_host")]
        par = [v[key] for k, v in legs.items() if k.startswith("parent_host")]
        rec = {"row": row, "host_route_fps": h[key], "device_route_fps": dv[key], "predicted_device_fps": pred,
               "achieved_over_predicted": dv[key] / pred, "device_over_host": dv[key] / h[key]}
        if par:
            rec["host_route_parent_commit_fps"] = par
            rec["host_route_this_tree_fps"] = new
            rec["host_new_over_parent"] = [min(new) / max(par), max(new) / min(par)]
        rec["legs"] = legs
        table.append(rec)
    res = {"what": "scripts/feed_rate.py on JPEG frames, merged by scripts/merge_feed_rate.py: FrameFeeder end to end (decode, pinned upload, GPU cubic "
                   "resize; batch 32), jpeg='host' against jpeg='device', same box, same session, same files",
           "gate_device_at_least_host": all(r["device_over_host"] >= 1 for r in table), "notes": notes, "rows": table}
    json.dump(res, open(out, "w"), indent=1)
    for r in table:
        print(r["row"], {k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items() if k != "legs"})


if __name__ == "__main__":
    main()
