"""Per-kernel VGPR / AGPR / scratch / LDS / occupancy of HIP sources (hipcc -Rpass-analysis):
one line per kernel with its full demangled name, sorted by name.

    python scripts/resource_usage.py SRC.hip [SRC.hip ...]

The build flags (and include root) come from the ddp_practice_amd package next to this
script, so a copy of the script inside another checkout measures that checkout."""
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, __file__.rsplit("/scripts", 1)[0])
from ddp_practice_amd import build as b  # noqa: E402


def kernels(src):
    with tempfile.NamedTemporaryFile(suffix=".o") as tmp:
        r = subprocess.run(["hipcc", "-x", "hip", *b._flags(), "--offload-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", tmp.name],
                           capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"compile failed: {src}\n{r.stderr[-4000:]}")
    cur, rows = None, []
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True,
                           text=True).stdout.splitlines()
    for row, n in zip(rows, names):
        row["name"] = n.strip()
    return rows


def main(argv):
    rows = [r for src in argv for r in kernels(src)]
    for row in sorted(rows, key=lambda r: r["name"]):
        print(f"v={row.get('VGPRs')} a={row.get('AGPRs')} scr={row.get('ScratchSize')} "
              f"lds={row.get('LDS Size')} occ={row.get('Occupancy')}  {row['name']}")


if __name__ == "__main__":
    main(sys.argv[1:])
