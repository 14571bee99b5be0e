"""Record tests/golden/igemm_bits.json: the sha256 of every output of every case of
tests/test_igemm_bits_gpu.py, computed with whichever ``ddp_practice_amd`` comes first on
PYTHONPATH -- a build of the commit the digests are to pin (the parent of a refactor):

    git archive <commit> | tar -x -C /some/dir && (cd /some/dir && python -m ddp_practice_amd.build)
    PYTHONPATH=/some/dir python scripts/record_igemm_bits.py --commit <commit> [--out FILE]

Every case runs twice; it is recorded only if both digests agree (a case that is not
run-to-run identical is listed under "unstable" and must be looked at, not dropped)."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded package was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "igemm_bits.json"))
    a = ap.parse_args()
    # the case list by file path: ``tests`` may also be a package of the tree on PYTHONPATH
    spec = importlib.util.spec_from_file_location("igemm_bits_cases",
                                                  os.path.join(ROOT, "tests", "test_igemm_bits_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    if not any(os.path.isdir(os.path.join(p, "ddp_practice_amd")) for p in sys.path if p):
        sys.path.append(ROOT)
    spec.loader.exec_module(mod)
    import ddp_practice_amd
    from ddp_practice_amd import _ext

    C = _ext.load()
    print(f"package: {os.path.dirname(ddp_practice_amd.__file__)}", flush=True)
    cases, unstable = {}, {}
    for cid, run in mod.CASES.items():
        d1, d2 = run(C), run(C)
        if d1 == d2:
            cases[cid] = d1
        else:
            unstable[cid] = [d1, d2]
        print(f"{cid}: {'ok' if d1 == d2 else 'UNSTABLE'} {d1[:16]}", flush=True)
    out = {"meta": {"parent_commit": a.commit, "torch_version_hip": torch.version.hip,
                    "device_name": torch.cuda.get_device_name(0)},
           "cases": cases}
    if unstable:
        out["unstable"] = unstable
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(cases)} cases, {len(unstable)} unstable -> {a.out}")
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
