"""What the time_*.py tools share: the two clocks, the one-run split into parts and the test sphere.  No tool imports from another tool."""
import time

import numpy as np
import torch

from ppsurf_amd import mcubes


def device_ms(fn, reps):
    """(median, min) ms of fn() between two device events, over `reps` runs after one warm-up (code objects, allocator)."""
    times = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def wall_ms(fn, reps):
    """(median, min) ms of fn() on the wall clock around a synchronise, over `reps` runs after one warm-up."""
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep > 0:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times))


def parts_of(run):
    """{part: ms} of one run of run(timer) with a synchronise between the parts: the stage calls timer(name) before every part."""
    parts, last = {}, [None, 0.0]

    def timer(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if last[0] is not None:
            parts[last[0]] = parts.get(last[0], 0.0) + (now - last[1]) * 1e3
        last[0], last[1] = name, now
    run(timer)
    timer(None)
    return parts


def sphere(R, dev):
    """(verts f32, faces) of the welded Marching Cubes mesh of an analytic sphere of radius 0.35 on an R^3 grid over [-0.5, 0.5]^3."""
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    return (verts * (1.0 / (R - 1)) - 0.5).float().contiguous(), faces.contiguous()
