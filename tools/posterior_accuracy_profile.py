"""profiles/r20_posterior_accuracy.txt from the output of `pytest tests/test_gpu_posterior.py -m gpu -s`:

    python tools/posterior_accuracy_profile.py PYTEST_OUTPUT [profiles/r20_posterior_accuracy.txt]

The tests print one `PO|path|measure|class|device|twin a|twin b|ratio` line per call and measure (the class with the worst ratio) and
one `PO|...|pair|...` line per pair of variants of one call.  This keeps, per route (the branches of csrc/evaluate.hip the call takes),
family and measure, the call with the worst device / max(twin a, twin b, floor), then the pair lines as they are."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import posterior_ref as pr  # noqa: E402


def main(log, out):
    best, pairs = {}, []
    for line in open(log):
        line = line.lstrip(".FEsx").rstrip("\n")          # the first line of a test follows pytest's progress character
        if not line.startswith("PO|"):
            continue
        r = line.split("|")
        if r[2] == "pair":
            pairs.append(line)
            continue
        path, q, cls, dev, ta, tb, ratio = r[1:8]
        fam, n, P, rest = re.match(r"(\w) n=(\d+) P=(\d+) (.*)$", path).groups()
        t = re.search(r"\[(.*)\]", rest)
        route = ", ".join(x.strip("' ") for x in t.group(1).split(",")) if t else "options: " + rest
        val = float(ratio.split()[1])
        key = (route, fam, q)
        if key not in best or val > best[key][0]:
            best[key] = (val, f"PO|{route}|{fam}|{q}|worst at n={n} P={P} class {cls}|{dev}|{ta}|{tb}|{ratio}")
    floors = " / ".join(f"{pr.FLOOR[q]:g}" for q in pr.MEASURES)
    fams = "; ".join(f"{f} {k} d={d} l={ell} noise {noise:g}" for f, (k, d, ell, noise) in pr.FAMILY.items())
    lines = [
        "# tests/test_gpu_posterior.py on an MI355X (pytest -m gpu -s), aggregated by tools/posterior_accuracy_profile.py: per route, family and"
        " measure the call with the worst device / max(twin a, twin b, floor)",
        "# PO|route (branches of csrc/evaluate.hip, as route() in the test names them)|family|measure|where|device|twin a|twin b(block width)|ratio",
        "# mu: |m - m_ref| / (eps (sum |k||alpha| + sigma^2 sum |alpha|)); nu: |v - v_ref| / (eps sigma^2);"
        " sig: |S - S_ref| / (eps (|w_p||w_q| + sigma^2)); reference in longdouble",
        "# twin a: scipy's float64 substitution; twin b: float64 numpy twin of the block-inverse sweep at the route's block width"
        f" (tests/posterior_ref.py); floors {floors}; the bar is ratio <= {pr.MARGIN:g}",
        f"# families (sigma^2 = {pr.SIG}): {fams}",
    ]
    lines += [best[k][1] for k in sorted(best)]
    lines.append("# pairs of variants of one call against each other: worst entry of S in eps sigma^2, then the variance and the entry of S"
                 " nearest their bar (the larger of the two routes' bars of the class); 0 = same bits")
    lines += pairs
    worst = collections.defaultdict(float)
    for (_, fam, q), (v, _) in best.items():
        worst[(fam, q)] = max(worst[(fam, q)], v)
    lines.append("# worst ratio per family and measure: " + "; ".join(f"{f} {q} {v:.3g}" for (f, q), v in sorted(worst.items())))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "r20_posterior_accuracy.txt"))
