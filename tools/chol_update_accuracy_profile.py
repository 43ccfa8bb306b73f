"""profiles/r21_chol_update_accuracy.txt from the output of `pytest tests/test_gpu_chol_update_accuracy.py -m gpu -s` and of
`pytest tests/test_chol_update_host.py -s`:

    python tools/chol_update_accuracy_profile.py GPU_OUTPUT HOST_OUTPUT [profiles/r21_chol_update_accuracy.txt]

The device tests print one `CU|route|family|n|k|class|phi dev/twin|rho dev/twin|lam dev/twin|ratios p r l` line per case (figures in
U = 2^-53, lam absolute; ratio = device / max(twin, floor)); the host test prints `CU host|...` lines.  This keeps, per route (the first
word of the case id: inst, edge, size, row0, class, family, ldl=.., set, crossing, strip, route, chain, facade) and family, the case with the
worst ratio of each measure, the twin's worst figures, and the host figures as they are."""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import chol_update_ref as cu  # noqa: E402


def _lines(path, prefix):
    for line in open(path):
        line = line.lstrip(".FEsx").rstrip("\n")              # the first line of a test follows pytest's progress character
        if line.startswith(prefix):
            yield line


def main(gpu_log, host_log, out):
    worst, twin, notes = {}, collections.defaultdict(lambda: [0.0, 0.0]), []
    for line in _lines(gpu_log, "CU|"):
        r = line.split("|")
        if "ratios " not in r[-1]:
            notes.append(line)
            continue
        route, fam = r[1].split(" ")[0].split("=")[0], r[2]
        ratios = [float(x) for x in r[-1].split()[1:]]
        for q, val in zip(("phi", "rho", "lam"), ratios):
            if (route, fam, q) not in worst or val > worst[route, fam, q][0]:
                worst[route, fam, q] = (val, line)
        for i in (0, 1):
            twin[route, fam][i] = max(twin[route, fam][i], float(r[6 + i].split("/")[1]))
    lines = [
        "# tests/test_gpu_chol_update_accuracy.py on an MI355X (pytest -m gpu -s), aggregated by tools/chol_update_accuracy_profile.py: per route,"
        " family and measure the case with the worst device / max(twin, floor)",
        "# CU|route and instantiation|family|n|k|class|phi device/twin|rho device/twin|lam device/twin|ratios phi rho lam",
        "# phi: worst row-wise relative error against the exact update (longdouble Householder, tests/chol_update_ref.py); rho: worst"
        " |L L^T + W W^T - L' L'^T|_ij / (nu_i nu_j); both in U = 2^-53; lam: absolute error of the log-determinant",
        f"# twin: the float64 numpy sweep of chol_update_ref; floors {cu.FLOOR_PHI / cu.U:g} U / {cu.FLOOR_RHO / cu.U:g} U / chol_ref.lam_floor;"
        f" the bar is ratio <= {cu.MARGIN}; caps on the twin (host test) phi {cu.CAP_PHI / cu.U:g} U, rho {cu.CAP_RHO / cu.U:g} U",
    ]
    for key in sorted(worst):
        lines.append(f"worst {key[2]}|" + worst[key][1])
    lines.append("# worst ratio per route and family (phi / rho / lam), and the twin's worst phi / rho in U")
    for route, fam in sorted({k[:2] for k in worst}):
        p, r, l = (worst[route, fam, q][0] for q in ("phi", "rho", "lam"))
        lines.append(f"{route}|{fam}|{p:.3g} / {r:.3g} / {l:.3g}|twin {twin[route, fam][0]:.3g} / {twin[route, fam][1]:.3g}")
    fams = collections.defaultdict(lambda: [0.0, 0.0, 0.0])
    for (route, fam, q), (v, _) in worst.items():
        i = ("phi", "rho", "lam").index(q)
        fams[fam][i] = max(fams[fam][i], v)
    summary = "# worst ratio per family: " + "; ".join(f"{f} {v[0]:.3g} / {v[1]:.3g} / {v[2]:.3g}" for f, v in sorted(fams.items()))
    lines.append(summary)
    lines.append("# bit properties and what the updated buffer is good for (logdet, potrs), as the tests printed them")
    lines += notes
    host = list(_lines(host_log, "CU host|"))
    per_case = [h for h in host if "|routes " in h]
    agree = max(float(h.split("|routes ")[1].split("|")[0]) for h in per_case)
    rounded = max(float(h.split("|rho rounded ")[1].split("|")[0]) for h in per_case)
    tphi = max(per_case, key=lambda h: float(h.split("|twin phi ")[1].split()[0]))
    trho = max(per_case, key=lambda h: float(h.split(" rho ")[-1].split()[0]))
    lines += ["# host (tests/test_chol_update_host.py -s), figures in U",
              f"# over {len(per_case)} cases: the two longdouble routes differ by at most {agree:.3g}; rho of the rounded reference at most {rounded:.3g}",
              "# the twin's worst phi: " + tphi, "# the twin's worst rho: " + trho]
    lines += [h for h in host if "|routes " not in h]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(summary)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "r21_chol_update_accuracy.txt"))
