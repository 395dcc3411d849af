#!/usr/bin/env python3
"""init_pinned_golden.json: sha256 of every initial parameter of the reference models behind model_golden.json (c2),
shapes_golden.json (c3, c4), variants_golden.json (mlp_gauss_tvf, mlp_disc) and tvf_mask_golden.json (sparsity,
window), drawn with MKL's LAPACK pinned to one code path: MKL_CBWR=COMPATIBLE on one thread.

The orthogonal initialiser is a QR factorisation; with MKL's default dispatch its last bits depend on the host CPU's
vector code path and on the thread count, so hashes taken that way only reproduce on a host like the one that made
them.  Pinned, the same seed gives the same bits on every x86 host (tests/test_model_init.py pins its own draws the
same way).

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_init_pinned_golden.py
The generators named above run unchanged in a scratch copy of this directory (nothing here is overwritten); only
the "params" hashes of their metadata are kept.
"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1"}


def main():
    env = dict(os.environ, **PINNED)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in glob.glob(os.path.join(HERE, "*.py")):
            shutil.copy(f, tmp)

        def run(*argv):
            subprocess.run([sys.executable, os.path.join(tmp, argv[0]), *argv[1:]], env=env, cwd=tmp, check=True)

        run("make_model_golden.py", "model")
        out["c2"] = json.load(open(os.path.join(tmp, "model_golden.json")))["params"]
        run("make_model_golden.py", "shapes")
        shapes = json.load(open(os.path.join(tmp, "shapes_golden.json")))
        out["c3"], out["c4"] = shapes["c3"]["params"], shapes["c4"]["params"]
        for tag in ("mlp_gauss_tvf", "mlp_disc"):
            run("make_variants_golden.py", tag)
            out[tag] = json.load(open(os.path.join("/tmp", f"variants_{tag}.npz.json")))[tag]["params"]
        run("make_tvf_mask_golden.py")
        masks = json.load(open(os.path.join(tmp, "tvf_mask_golden.json")))
        out["sparsity"], out["window"] = masks["sparsity"]["params"], masks["window"]["params"]
    doc = {"mkl_env": PINNED,
           "params": {tag: {n: {"shape": p["shape"], "sha256": p["sha256"]} for n, p in ps.items()}
                      for tag, ps in out.items()}}
    json.dump(doc, open(os.path.join(HERE, "init_pinned_golden.json"), "w"), indent=1)
    print("init_pinned_golden:", {tag: len(ps) for tag, ps in doc["params"].items()})


if __name__ == "__main__":
    main()
