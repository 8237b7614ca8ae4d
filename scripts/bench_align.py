"""Times the rigid alignment to the baked field (d3f_volume_align_*, csrc/align_kernels.hip; BakedField.align) on the synthetic smooth scene (needs
an MI355X) and writes profiles/align/results.txt.  One run, no thresholds: the file reports, nothing is asserted, and nothing was tuned.

Method of scripts/bench_peaks.py: HIP events on the stream round the call, median of --runs runs after warm-up; the header carries the date, the
commit and the shader clock.  The problem: n surface points of the 4 mm bake of the work box as the model at the identity, their descriptors
sampled from the field as targets, I instances that start from the truth moved by 2 degrees about a random axis and 1 voxel along a random
direction.  I = 1 / 64 / 4096, n = 32 / 1024, C = 3 / 64 / 384 (a 3- and a 64-component head and the 384 channels themselves), dense and as a
band of 12 mm; a combination whose targets would hold more than 2^28 floats is skipped and listed.  Per line, measured in the same run:

    accumulate  one d3f_volume_align_accumulate with the per-instance fold (BakedField.normal_equations without its Python around it)
    align       BakedField.align(iters=10): 22 launches and the Python around them; with how many instances ended CONVERGED and the mean cost
    adam        100 Adam steps (lr 1e-3 on log-rotation and translation) on the same sum of squared residuals through BakedField.eval's
                autograd: the recipe this replaces, parent-commit code; above 2^24 points x channels 10 steps are timed and scaled by 10

    python scripts/bench_align.py [--runs 5] [--out profiles/align/results.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402
from d3fields_amd.rigid import rigid_transform, so3_exp_map     # noqa: E402

BAND = 0.012
STEP = 0.004
INSTANCES = (1, 64, 4096)
POINTS = (32, 1024)
MAX_TARGET_FLOATS = 1 << 28
ADAM_FULL = 1 << 24


def fmt(t):
    return "median %9.4f ms (min %.4f, max %.4f)" % t


def starts(I, centre, dev, gen):
    """row-vector poses: the identity moved by 2 degrees about the points' centre and one voxel"""
    axis = torch.nn.functional.normalize(torch.randn(I, 3, generator=gen), dim=1)
    rot = so3_exp_map(axis * (2.0 * torch.pi / 180.0))
    shift = torch.nn.functional.normalize(torch.randn(I, 3, generator=gen), dim=1) * STEP
    trans = centre[None] - (centre[None, None] @ rot)[:, 0] + shift          # p @ rot + trans turns about the centre
    return rot.to(dev).contiguous(), trans.to(dev).contiguous()


def adam_steps(field, name, pts, targets, rot0, trans0, steps):
    I, n = pts.shape[:2]
    log_r = torch.zeros(I, 3, device=pts.device, requires_grad=True)
    t = trans0.clone().requires_grad_(True)
    opt = torch.optim.Adam([log_r, t], lr=1e-3)
    loss = None
    for _ in range(steps):
        cur = rigid_transform(pts, torch.bmm(rot0, so3_exp_map(log_r)), t).reshape(-1, 3)
        out = field.eval(cur, return_names=[name])
        loss = (out["dist"] ** 2 * out["valid_mask"]).sum() + (((out[name] - targets.reshape(I * n, -1)) ** 2).sum(dim=1) * out["valid_mask"]).sum()
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, 384, seed=1).to(dev)
    f.H, f.W = H, W
    f.add_projection("head3", components=torch.randn(3, 384, generator=torch.Generator().manual_seed(2)))
    f.add_projection("head64", components=torch.randn(64, 384, generator=torch.Generator().manual_seed(3)))
    _, shell = f.grid_shell(synth.WORK_BOX, STEP)
    lines = ["rigid alignment to the baked field (d3f_volume_align_*; BakedField.align), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, one run, nothing tuned; device times: HIP events round the call, median of %d runs after 3 warm-up calls (min, max); adam: one run; "
             "scene: synth smooth, %d views of %d x %d, step %g m, %d shell points; starts 2 degrees and 1 voxel off" % (args.runs, V, H, W, STEP, shell.shape[0]), ""]

    def flush():
        text = "\n".join(lines[:1] + [clock_line()] + lines[1:]) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        return text

    skipped = []
    for name in ("head3", "head64", "dino_feats"):
        dense = f.bake(synth.WORK_BOX, STEP, return_names=[name])
        C = dense._sets[name].shape[3]
        for banded in (False, True):
            field = dense.to_band(BAND) if banded else dense
            nx, ny, nz = field.grid_shape
            lines.append("C = %d (%s), %d x %d x %d, %s" % (C, name, nx, ny, nz, "band of %g m: %.2f %% of the voxels stored" % (BAND, 100 * field.stored_fraction) if banded
                                                          else "dense"))
            for n in POINTS:
                pick = torch.randperm(shell.shape[0], generator=gen)[:n].to(dev)
                model = shell[pick].contiguous()
                with torch.no_grad():
                    row = field.eval(model, return_names=[name])[name]
                for I in INSTANCES:
                    if I * n * C > MAX_TARGET_FLOATS:
                        skipped.append("C = %d, I = %d, n = %d%s" % (C, I, n, ", band" if banded else ""))
                        continue
                    pts = model[None].expand(I, n, 3).contiguous()
                    targets = row[None].expand(I, n, C).contiguous()
                    rot, trans = starts(I, model.mean(dim=0).cpu(), dev, gen)
                    t_acc = median_ms(lambda: field.normal_equations(pts, rot, trans, name=name, targets=targets), args.runs, 1)
                    fit = field.align(pts, name, targets, rot=rot, trans=trans, iters=10)
                    t_fit = median_ms(lambda: field.align(pts, name, targets, rot=rot, trans=trans, iters=10), args.runs, 1)
                    steps = 100 if I * n * C <= ADAM_FULL else 10
                    loss = []
                    t_adam = median_ms(lambda: loss.append(adam_steps(field, name, pts, targets, rot, trans, steps)), 1, 1, warmup=0)
                    scale = 100 // steps
                    lines.append("    I = %4d, n = %4d: normal_equations %s; align %s, %d of %d CONVERGED, mean cost %.3g -> %.3g; adam 100 steps %9.2f ms%s, mean loss %.3g"
                                 % (I, n, fmt(t_acc), fmt(t_fit), int((fit["status"] == 1).sum()), I, float(fit["history"][:, 0].mean()), float(fit["cost"].mean()),
                                    t_adam[0] * scale, " (10 timed, x 10)" if scale > 1 else "", float(loss[-1]) / I))
                    flush()
                    del pts, targets, fit, loss
                    torch.cuda.empty_cache()
            del field
        del dense
        torch.cuda.empty_cache()
    lines.append("")
    lines.append("skipped (targets above 2^28 floats): %s" % ("; ".join(skipped) if skipped else "none"))
    print(flush())


if __name__ == "__main__":
    main()
