"""What the map of a gridded window costs: `Context.map_draw` -- rasterised and coded on the device --
beside the reference's matplotlib calls on the same arrays (s3:502-519, 716-718).

    python tools/map_picture.py [--vectors 1000000] [--host-vectors 100000] [--reps 10] [--out profiles/map_picture.txt]

A synthetic fjord of about 600 cells of 200 m and a window of --vectors velocity vectors, uploaded once
(`map_arrows_set`), gridded on the device (`bin_velocities`), then for the one-map and the two-map picture at 1400 pixels:
  wall     the whole call, host clock, the call waits for the device: best / median / worst of --reps after 3 warm-up calls
  kernels  HIP events around every kernel of the call (icelk_prof_enable), in a run of the same calls of its own: the
           average per launch of the map kernels, the forward kernel and the coder's kernels
  host     where matplotlib is present: the reference's PolyCollection and quiver calls on the same arrays -- the gridded
           arrows, and --host-vectors of the vectors (quiver of 10^6 arrows takes minutes) --, PNG at 100 dpi into memory
One JSON line per picture on stdout; --out writes them to a file as well.  Needs a GPU."""
import argparse
import datetime as dt
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def scene(n, seed=7):
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, 60, endpoint=False)
    rad = 2400 + 500 * np.sin(3 * ang) + rng.uniform(-150, 150, 60)
    fjord = {"x": 500000.0 + np.round(1.5 * rad * np.cos(ang), 1), "y": 7000000.0 + np.round(rad * np.sin(ang), 1)}
    x = rng.uniform(fjord["x"].min(), fjord["x"].max(), n)
    y = rng.uniform(fjord["y"].min(), fjord["y"].max(), n)
    flow = 0.25 * (1 + np.sin((x - 500000.0) / 1500.0))
    u, v = flow + rng.normal(0, 0.03, n), 0.3 * flow + rng.normal(0, 0.03, n)
    return fjord, x, y, u, v


def host_route(fjord, r, grid_size, limits, vectors, two, vmax):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.collections import PolyCollection
    from iceberg_tracking_code_amd import scaled_arrows
    t0 = time.perf_counter()
    plt.ioff()
    fig, axes = plt.subplots(1, 2 if two else 1, figsize=(28 if two else 14, 10.75), facecolor="w")
    ax1 = axes[1] if two else axes
    ax1.add_collection(PolyCollection(r["measured"], color="none", linewidths=0.5, edgecolor="darkgray"))
    ax1.add_collection(PolyCollection(r["not_measured"], color="lightgray", linewidths=0.5, edgecolor="darkgray"))
    du, dv = scaled_arrows(r["u"], r["v"]) if two else scaled_arrows(r["u"], r["v"], exponent=0.2, factor=100)
    q = ax1.quiver(r["x"], r["y"], du, dv, r["speed"], clim=[0.0, vmax], pivot="mid", cmap="gist_rainbow", units="x", scale=1,
                   width=8 if two else 4, alpha=1, zorder=1000)
    if two:
        q = axes[0].quiver(vectors[:, 0], vectors[:, 1], vectors[:, 2], vectors[:, 3], vectors[:, 4], clim=[0.0, vmax], cmap="gist_rainbow",
                           units="x", scale=1.0, width=3.5, alpha=0.75)
    for ax in (axes if two else [axes]):
        ax.plot(fjord["x"], fjord["y"], "-", lw=0.6, color="k")
        fig.colorbar(q, ax=ax)
        ax.set_xlim(limits[:2])
        ax.set_ylim(limits[2:])
    fig.tight_layout()
    buf = io.BytesIO()
    plt.savefig(buf, format="png", dpi=100)
    plt.close(fig)
    return 1e3 * (time.perf_counter() - t0), len(buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1000000)
    ap.add_argument("--host-vectors", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--width", type=int, default=1400)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from iceberg_tracking_code_amd import Context, bin_velocities, map_picture, map_strings, map_view
    fjord, x, y, u, v = scene(a.vectors)
    day = dt.datetime(2019, 7, 24)
    strings = map_strings(day, day + dt.timedelta(hours=10), day + dt.timedelta(hours=10.5), ["cam1", "cam2"], a.grid)
    cams = [(float(fjord["x"].min()) + 200.0, float(fjord["y"].min()) + 200.0), (float(fjord["x"].max()) - 300.0, float(fjord["y"].max()) - 100.0)]
    lines = []
    with Context(64, 64, n_slots=1, max_pts=1 << 18) as ctx:
        r = bin_velocities(ctx, x, y, u, v, fjord, a.grid, 3)
        vectors = np.column_stack([x, y, u * 60.0, v * 60.0, np.hypot(u, v)])
        t0 = time.perf_counter()
        ctx.map_arrows_set(vectors, np.zeros(len(vectors), np.int32))
        upload_ms = 1e3 * (time.perf_counter() - t0)
        for switch in (1, 2):
            pic = map_picture(fjord, a.grid, r["measured"], r["not_measured"], r["x"], r["y"], r["u"], r["v"], r["speed"], strings, cameras=cams,
                              label=cams[0], n_camnames=2, plot_switch=switch, group=0, out_width=a.width, quality=a.quality)
            for _ in range(3):
                data = ctx.map_draw(pic)
            wall = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.map_draw(pic)
                wall.append(1e3 * (time.perf_counter() - t0))
            ctx.prof_reset()
            ctx.prof_enable(True)
            for _ in range(a.reps):
                ctx.map_draw(pic)
            ctx.prof_enable(False)
            prof = ctx.prof_table()
            table = {k: round(w["avg_us"], 2) for k, w in prof.items() if k.startswith(("map_", "jpeg_fwd", "jpeg_enc_"))}
            launches = {k: prof[k]["launches"] // a.reps for k in table}
            res = dict(tool="map_picture", plot_switch=switch, picture=[pic["width"], pic["height"]], cells=len(r["measured"]) + len(r["not_measured"]),
                       measured=len(r["measured"]), vectors=int(a.vectors) if switch == 2 else 0, quality=a.quality, file_bytes=len(data), reps=a.reps,
                       arrows_upload_ms=round(upload_ms, 2),
                       wall_ms=dict(best=round(min(wall), 3), median=round(statistics.median(wall), 3), worst=round(max(wall), 3)),
                       kernel_avg_us=table, kernel_launches_per_call=launches,
                       kernels_us_per_call=round(sum(table[k] * launches[k] for k in table), 1),
                       map_kernels_us_per_call=round(sum(table[k] * launches[k] for k in table if k.startswith("map_")), 1))
            try:
                n_host = min(a.host_vectors, a.vectors)
                host = [host_route(fjord, r, a.grid, map_view(fjord, switch), vectors[:n_host], switch == 2, 0.5) for _ in range(2)]
                res["host_route"] = dict(vectors=n_host if switch == 2 else 0, matplotlib_ms=[round(h[0], 1) for h in host], png_bytes=host[-1][1])
            except ImportError:
                res["host_route"] = "not measured: matplotlib is not installed"
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
