"""Stream time of the ray caster's three ways to draw 100 frames (DESIGN §5f's table): one env of the 27-dof task, at 320 x 240 and 640 x 480
with 1, 2 and 4 samples per axis —
    eager     100 x Renderer.render()        (refresh + pose + rays)
    capture   100 x Trajectory.capture()     (refresh + pose-anchor)
    batched   cast_frames over the 100 recorded frames (pp_render_rays_frames, `launches` launches)
— stream events around each, best of --repeats.  One JSON line per row.  Needs a GPU.

    python tools/render_bench.py [--tree NAME]
    rocprofv3 --kernel-trace --stats -d out -o render -- python tools/render_bench.py --repeats 1      # the launches' own time
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASK = "HumanoidPingpongTiltNESSparse27DOFG1"
SIZES = ((320, 240), (640, 480))
SAMPLES = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="a label copied into every line (which checkout this is)")
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    import isaacgym_amd
    from isaacgym_amd import render
    task = isaacgym_amd.make(seed=1, task=TASK, num_envs=args.num_envs)
    gen = torch.Generator(device=task.device).manual_seed(3)
    for _ in range(8):                                                                    # off the reset pose
        task.step(torch.rand((task.num_envs * task.num_agents, task.num_actions), device=task.device, generator=gen) * 2 - 1)
    F = args.frames

    def best_ms(fn):
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return round(min(out), 4)

    for w, h in SIZES:
        for s in SAMPLES:
            r = render.Renderer(task, envs=(0,), width=w, height=h, samples=s)
            traj = render.Trajectory(r, length=F)
            out = torch.zeros((F, 1, h, w, 4), dtype=torch.uint8, device=task.device)

            def eager():
                for _ in range(F):
                    r.render()

            def capture():
                for _ in range(F):
                    traj.capture()

            def batched():
                render.cast_frames(r.L, r.scene.header, r._cam, traj.posed, traj.anchor, s, out)

            eager(), capture(), batched()                                                 # warm-up: code objects, allocator
            row = dict(tree=args.tree, task=TASK, width=w, height=h, samples=s, frames=F, repeats=args.repeats, eager_ms=best_ms(eager),
                       capture_ms=best_ms(capture), batched_ms=best_ms(batched), launches=-(-F // render.launch_frames(s, 1, w, h)))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
