"""Golden film geometry of the reference's top-down renderer (runs only where the reference's source tree is available).

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tools/gen_render_geometry.py  ->  tests/golden/render_bbox_v0.json

The reference's TopDownRenderer (obs/top_down_renderer.py) fits its film to `RoadNetwork.get_bounding_box()`
(component/road/road_network.py:105-118).  This tool builds the reference's own road networks through the stubs of
oracle/ref_export.py (nothing under oracle/ changes) and records that bounding box, (x_min, x_max, y_min, y_max):
  pg   PGDrive-v0, seeds 1000..1099 (map=3, lane_num=3, lane_width=3.5, exit_length=50)
  ma   the five multi-agent maps (roundabout, intersection, bottleneck, tollgate, parking lot) at their env defaults
pgdrive_amd/render.py restates the box from the lane descriptions the engine holds; tests/test_render_cpu.py compares.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import ref_export  # noqa: E402  (installs the stubs for panda3d / gym / ...)


def main():
    out = dict(version=0, source="decisionforce/pgdrive v0.1.4 RoadNetwork.get_bounding_box(): [x_min, x_max, y_min, y_max]",
               pg={}, ma={})
    for seed in range(1000, 1100):
        m = ref_export.generate(seed, block_num=3)
        out["pg"][str(seed)] = [float(v) for v in m["net"].get_bounding_box()]
    for name, fn in (("roundabout", ref_export.generate_ma_roundabout), ("intersection", ref_export.generate_ma_intersection),
                     ("bottleneck", ref_export.generate_ma_bottleneck), ("tollgate", ref_export.generate_ma_tollgate),
                     ("parking_lot", ref_export.generate_ma_parking_lot)):
        m = fn()
        out["ma"][name] = [float(v) for v in m["net"].get_bounding_box()]
    path = os.path.join(ROOT, "tests", "golden", "render_bbox_v0.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
