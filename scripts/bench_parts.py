"""Times descriptor-gated links and the labelling over them (d3f_volume_links, csrc/parts_kernels.hip; d3f_volume_components_linked;
BakedField.links / parts) on the synthetic smooth scene (needs an MI355X) and writes profiles/parts/results.txt.  No thresholds: the file
reports, nothing is asserted.

Method of scripts/bench_pool.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the commit and
the shader clock.  Configurations: the 200 x 175 x 55 bake (4 mm) with a dense 384-channel set; its 5-mm band; the 1-mm grid of the same box
with the 384 channels in a band of two steps; an 8-channel instance-mask set under the argmax rule.  Sites are valid & dist <= one step, the
rows are random numbers (three prototypes plus noise, so that links both hold and fail) -- the time of the link kernel does not depend on
them.  Next to every time, measured in the same run:

    copy    a bare index_select copy of exactly the member rows: every member row has to be read once
    torch   the recipe links() replaces, where it fits in memory: per offset a shifted difference of the [nx, ny, nz, C] array, squared, summed
            and compared (dense fields only; 13 temporaries of the row array's size)

    python scripts/bench_parts.py [--runs 10] [--out profiles/parts/results.txt]
"""
import argparse
import datetime
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from bench_pool import with_set     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402

OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))[:13]


def torch_links(rows, member, t2):
    """the shifted-difference recipe on a dense [nx, ny, nz, C] array -> int32 bits (the sums are torch's, not the contract's order)"""
    nx, ny, nz, _ = rows.shape
    out = torch.zeros((nx, ny, nz), dtype=torch.int32, device=rows.device)
    for j, off in enumerate(OFFSETS):
        hi = tuple(slice(1, n) if d < 0 else slice(0, n - 1) if d > 0 else slice(None) for n, d in zip((nx, ny, nz), off))
        lo = tuple(slice(0, n - 1) if d < 0 else slice(1, n) if d > 0 else slice(None) for n, d in zip((nx, ny, nz), off))
        ok = ((rows[hi] - rows[lo]).square_().sum(-1) <= t2) & member[hi] & member[lo]
        out[hi] |= ok.int() << j
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["descriptor-gated links (d3f_volume_links) and parts, %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, one run; HIP events, median of %d runs after 3 warm-up calls (min, max); scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W), ""]
    # (name, step, band or None, channels, rule keywords)
    configs = [("4-mm dense, C = 384, l2", 0.004, None, 384, {"rule": "l2", "tau": 6.0}),
               ("4-mm grid, 5-mm band, C = 384, l2", 0.004, 0.005, 384, {"rule": "l2", "tau": 6.0}),
               ("4-mm dense, C = 384, cosine", 0.004, None, 384, {"rule": "cosine", "cos": 0.8}),
               ("1-mm grid, 2-mm band, C = 384, l2", 0.001, 0.002, 384, {"rule": "l2", "tau": 6.0}),
               ("4-mm dense, mask set C = 8, argmax", 0.004, None, 8, {"rule": "argmax"})]
    bakes = {}
    for name, step, band, C, rule in configs:
        if step not in bakes:
            bakes.clear()
            torch.cuda.empty_cache()
            bakes[step] = f.bake(synth.WORK_BOX, step, return_names=[])
        base = bakes[step]
        nx, ny, nz = base.grid_shape
        n = nx * ny * nz
        mark = None if band is None else base._mark(band)
        rows_n = n if band is None else int(mark[2].shape[0])
        if 4 * rows_n * C > 0.45 * torch.cuda.mem_get_info(dev)[0]:
            lines.append("%s: the rows alone are %.1f GB -- not run" % (name, 4 * rows_n * C / 1e9))
            continue
        gen = torch.Generator(device=dev).manual_seed(17)
        proto = torch.randn((3, C), device=dev, generator=gen)
        rows = proto[torch.randint(0, 3, (rows_n,), device=dev, generator=gen)] + 0.2 * torch.randn((rows_n, C), device=dev, generator=gen)
        field = with_set(base, "feat", rows.view(nx, ny, nz, C)) if band is None else with_set(base, "feat", rows, mark, band)
        iso = step
        members = field._members(field._site_mask("bench", iso, "free", None))
        m = int(members.sum())
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 3)
        lmed, llo, lhi = median_ms(lambda: field.links("feat", iso=iso, **rule), runs, 1)
        lk = field.links("feat", iso=iso, **rule)
        bits = int(sum(((lk.view(torch.int16).int() >> j) & 1).sum() for j in range(13)))
        pmed, plo, phi = median_ms(lambda: field.parts("feat", iso=iso, **rule), runs, 1)
        parts = field.parts("feat", iso=iso, **rule)
        cmed, _, _ = median_ms(lambda: field.components(iso=iso), runs, 1)
        lines.append("%s: %d x %d x %d = %.2f M voxels, %d rows stored, %d members, %d links set, %d parts (components(): %d)"
                     % (name, nx, ny, nz, n / 1e6, rows_n, m, bits, parts.found, field.components(iso=iso).found))
        lines.append("    links %9.3f ms (min %.3f, max %.3f)    parts %9.3f ms (min %.3f, max %.3f)    components() alone %.3f ms" % (lmed, llo, lhi, pmed, plo, phi, cmed))
        at = members.view(-1).nonzero().view(-1) if band is None else field.slot.view(-1)[members.view(-1)].long()
        gb = 4.0 * m * C / 1e9
        ymed, ylo, yhi = median_ms(lambda: rows.index_select(0, at), runs, 1)
        text = "    copy of the %.3f GB of member rows: %.3f ms (min %.3f, max %.3f)" % (gb, ymed, ylo, yhi)
        if band is None and rule["rule"] == "l2" and 3 * 4 * n * C < 0.8 * torch.cuda.mem_get_info(dev)[0]:
            t2 = float(rule["tau"]) ** 2
            tmed, tlo, thi = median_ms(lambda: torch_links(field._sets["feat"], members, t2), max(3, runs // 3), 1, warmup=1)
            text += "    torch shifted differences: %.3f ms (min %.3f, max %.3f)" % (tmed, tlo, thi)
        elif band is not None:
            text += "    torch shifted differences: the rows are compacted, the recipe needs the dense [n, C] array (%.1f GB)" % (4.0 * n * C / 1e9)
        lines.append(text)
        lines.append("")
        del field, rows, lk, parts, members, at
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
