"""profiles/rescue64_edges.json from the figures tests/test_gpu_rescue64.py reports.

  ALS_TEST_REPORT=errors.jsonl python -m pytest tests/test_gpu_rescue64.py -m gpu
  python tools/rescue64_profile.py errors.jsonl WALL_SECONDS [profiles/rescue64_edges.json]

One entry per case (helpers.report lines whose name starts with "rescue64["); WALL_SECONDS is
what pytest printed for the whole file.  The summary is computed from the entries."""
import json
import sys


def build(lines, wall_s):
    res = {}
    for line in lines:
        r = json.loads(line)
        if r["test"].startswith("rescue64["):
            res[r["test"]] = r["value"]
    errs = {k: v["max_rel_err"] for k, v in res.items() if "max_rel_err" in v}
    worst = max(errs, key=errs.get)
    guards = [v for v in res.values() if "unlisted_rows_max_rel_err" in v]
    return {
        "source": "pytest -m gpu tests/test_gpu_rescue64.py with ALS_TEST_REPORT (MI355X), "
                  "assembled by tools/rescue64_profile.py; one entry per case",
        "cases": len(res),
        "wall_s_whole_file": wall_s,
        "summary": {
            "bar": 2.0 ** -23,
            "worst_max_rel_err": errs[worst],
            "worst_case": worst,
            "rank_cond_eps_bar": 2.0 ** -30,
            "worst_rank_cond_eps": max(v["rank_cond_eps"] for v in res.values()),
            "longest_list": max(v["list_length"] for v in res.values()),
            "shortest_list": min(v["list_length"] for v in res.values()),
            "worst_unlisted_rows_max_rel_err": max(v["unlisted_rows_max_rel_err"] for v in guards),
            "worst_unlisted_rows_yardstick_ratio": max(
                v["unlisted_rows_max_rel_err"] / v["unlisted_rows_textbook_max_rel_err"]
                for v in guards),
        },
        "results": res,
    }


if __name__ == "__main__":
    out = sys.argv[3] if len(sys.argv) > 3 else "profiles/rescue64_edges.json"
    with open(sys.argv[1]) as f:
        prof = build(f, float(sys.argv[2]))
    with open(out, "w") as f:
        json.dump(prof, f, indent=1)
        f.write("\n")
    print(json.dumps(prof["summary"], indent=1))
