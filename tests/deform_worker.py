"""Worker of tests/test_deform.py: one rank of a multi-process run over the gloo transport (as tests/pressure_worker.py).

    python deform_worker.py <rank> <world> <port> <px> <py> <pz> <mode> <json list of CLI flags> <json job>

mode "host": a host-only simulation; set_box(job["box"]) and print the geometry this rank holds (no device is touched).
mode "gpu":  the HIP path on device 0; strain at job["rates"] for job["steps"] steps, then deform(job["scale"]); print energy, virial and box.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    grid = [int(v) for v in sys.argv[4:7]]
    mode = sys.argv[7]
    args = json.loads(sys.argv[8]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    job = json.loads(sys.argv[9])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    if mode == "gpu":
        pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args, host_only=(mode == "host"))
    if mode == "host":
        sim.set_box(job["box"])
        lo, hi = sim.local_bounds()
        out = {"box": [float.hex(v) for v in sim.box], "lo": [float.hex(v) for v in lo], "hi": [float.hex(v) for v in hi]}
    else:
        sim.set_strain_rate(job["rates"])
        sim.step(job["steps"])
        sim.set_strain_rate([0.0, 0.0, 0.0])
        sim.deform(job["scale"])
        sim.sum_atoms()
        w, k = sim.virial()
        out = {"box": [float.hex(v) for v in sim.box], "energy": list(sim.energy()), "w": w.tolist(), "k": k.tolist()}
    print("DEFORM", json.dumps(out))
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
