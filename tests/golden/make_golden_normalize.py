"""Generate tests/golden/normalize_golden.npz and tests/golden/normalize_web30k.json from the REAL reference on CPU: two small three-role
libsvm data sets are written to a temporary directory and run through the reference's own reproducibility/normalize_features.py in a
child process; the raw arrays and the script's ``_normalized`` output (parsed back with scikit-learn, fp64) are stored.

Every raw value is exactly representable in fp32 (integers and dyadic fractions), so the script's fp64 parse and the device's fp32 parse
hold the same numbers; no zero is negative, so a file that leaves zeros out parses back to the same bits.

Case "a": 12 features, 20 / 7 / 6 queries (train / test / vali) of 1 to 8 items, run with
``--features_without_logarithm 1 4 --features_negative 6 7``.  Columns (zero-based):
     0  counts                                  log
     1  signed eighths, in the without-log list standardised only
     2  the constant 3                          log; std 0: the script's output is cancellation noise over eps
     3  all zero                                log; std 0
     4  counts up to 2^20, without-log list     standardised only
     5  2^-k, k = 0 .. 10                       log
     6  negative list, truly <= 0               negated, log
     7  negative list, mixed signs              negated, NO log (the script prints its message)
     8  >= 0 in train and test, one negative in vali     NO log: the decision is taken over all three roles
     9  2^k, k = 0 .. 20                        log
    10  >= 0 in train and vali, one negative in test     NO log -- and the ONLY column whose decision changes when test.txt is absent
    11  counts >= 1                             log; non-zero in every row, so every file states all 12 features
Case "b": 136 features, 6 queries of 4 items per role, run with NO list arguments (the script's defaults = normalize_web30k.json).
Columns 20 and 113 hold a negative value of s x in train, so two default-log columns lose the logarithm.

normalize_web30k.json: the script's argparse defaults and its two epsilons, read from its source text (the function ``parse_args`` is
executed on its own; the module is never imported: it runs on import).

    python tests/golden/make_golden_normalize.py        # build container only
"""
import ast
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import REFERENCE_ROOT  # noqa: E402
from tests import featnorm_ref as R  # noqa: E402

SCRIPT = os.path.join(REFERENCE_ROOT, "reproducibility", "normalize_features.py")
CASE_A_LISTS = ([1, 4], [6, 7])
ONLY_TEST_DECIDES = [10]                       # case "a": the columns whose log decision changes when test.txt is absent


def _queries(rng, n_queries, lo, hi, first_qid):
    lens = rng.randint(lo, hi + 1, n_queries)
    return np.repeat(np.arange(first_qid, first_qid + n_queries), lens)


def case_a():
    rng = np.random.RandomState(20240)
    out = {}
    for role, nq, q0 in (("train", 20, 1), ("test", 7, 101), ("vali", 6, 201)):
        qid = _queries(rng, nq, 1, 8, q0)
        n = len(qid)
        x = np.zeros((n, 12))
        x[:, 0] = rng.randint(0, 50, n)
        x[:, 1] = rng.randint(-32, 33, n) / 8.0
        x[:, 2] = 3.0
        x[:, 4] = rng.randint(0, 2 ** 20 + 1, n)
        x[:, 5] = 2.0 ** -rng.randint(0, 11, n)
        x[:, 6] = 0.0 - rng.randint(0, 40, n)
        x[:, 7] = rng.randint(-20, 21, n)
        x[:, 8] = rng.randint(0, 30, n)
        x[:, 9] = 2.0 ** rng.randint(0, 21, n)
        x[:, 10] = rng.randint(0, 16, n) / 4.0
        x[:, 11] = rng.randint(1, 100, n)
        if role == "train":
            x[0, 4], x[1, 5], x[2, 9], x[3, 5] = 2.0 ** 20, 2.0 ** -10, 2.0 ** 20, 1.0
        if role == "vali":
            x[n // 2, 8] = -2.0
        if role == "test":
            x[n - 1, 10] = -0.25
        out[role] = (x.astype(np.float32), rng.randint(0, 5, n), qid)
    return out


def case_b():
    rng = np.random.RandomState(20241)
    without, negative = read_settings()["features_without_logarithm"], read_settings()["features_negative"]
    out = {}
    for role, q0 in (("train", 1), ("test", 101), ("vali", 201)):
        qid = _queries(rng, 6, 4, 4, q0)
        n = len(qid)
        x = rng.randint(0, 400, (n, 136)) / 4.0
        x[:, without] = rng.randint(-400, 401, (n, len(without))) / 4.0
        x[:, negative] = 0.0 - rng.randint(0, 400, (n, len(negative))) / 4.0
        x[:, 135] = rng.randint(1, 60, n)
        if role == "train":
            x[5, 20], x[7, 113] = -1.5, 2.0
        out[role] = (x.astype(np.float32), rng.randint(0, 5, n), qid)
    return out


def read_settings():
    """the script's default lists and epsilons, from its source"""
    with open(SCRIPT) as fh:
        tree = ast.parse(fh.read())
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "parse_args"]
    consts = {t.id: node.value.value for node in tree.body if isinstance(node, ast.Assign) and isinstance(node.value, ast.Constant)
              for t in node.targets if isinstance(t, ast.Name)}
    from argparse import ArgumentParser, Namespace
    ns = {"ArgumentParser": ArgumentParser, "Namespace": Namespace}
    exec(compile(ast.Module(body=fn, type_ignores=[]), SCRIPT, "exec"), ns)
    argv, sys.argv = sys.argv, ["normalize_features.py", "--ds_path", "."]
    try:
        args = ns["parse_args"]()
    finally:
        sys.argv = argv
    return {"features_without_logarithm": [int(i) for i in args.features_without_logarithm],
            "features_negative": [int(i) for i in args.features_negative], "eps_log": float(consts["eps_log"]), "eps": float(consts["eps"])}


def run_reference(roles, lists, tmp):
    """{role: normalised fp64 array}, and the columns the script's message names"""
    from sklearn.datasets import load_svmlight_file
    ds = os.path.join(tmp, "ds")
    os.makedirs(ds)
    for role, (x, y, qid) in roles.items():
        R.write_libsvm(os.path.join(ds, role + ".txt"), x, y, qid)
    cmd = [sys.executable, SCRIPT, "--ds_path", ds]
    if lists is not None:
        cmd += ["--features_without_logarithm"] + [str(i) for i in lists[0]] + ["--features_negative"] + [str(i) for i in lists[1]]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"),
                          cwd=tmp).stdout.decode()
    lost = [int(m) for m in re.findall(r"feature no\. (\d+) are still < 0", text)]
    F = next(iter(roles.values()))[0].shape[1]
    out = {}
    for role in roles:
        xn, _, _ = load_svmlight_file(os.path.join(ds + "_normalized", role + ".txt"), query_id=True, n_features=F)
        out[role] = np.asarray(xn.toarray(), dtype=np.float64)
    return out, lost


def build():
    settings = read_settings()
    out = {}
    for name, roles, lists in (("a", case_a(), CASE_A_LISTS), ("b", case_b(), None)):
        with tempfile.TemporaryDirectory() as tmp:
            normalized, lost = run_reference(roles, lists, tmp)
        used = lists if lists is not None else (settings["features_without_logarithm"], settings["features_negative"])
        out[name + ".features_without_logarithm"] = np.asarray(used[0], dtype=np.int64)
        out[name + ".features_negative"] = np.asarray(used[1], dtype=np.int64)
        out[name + ".no_log_negative"] = np.asarray(lost, dtype=np.int64)
        for role, (x, y, qid) in roles.items():
            assert np.array_equal(x.astype(np.float64).astype(np.float32), x) and (x[:, -1] != 0).all() and not np.signbit(x[x == 0]).any()
            out["%s.%s.x" % (name, role)], out["%s.%s.y" % (name, role)], out["%s.%s.qid" % (name, role)] = x, y.astype(np.int64), qid.astype(np.int64)
            out["%s.%s.normalized" % (name, role)] = normalized[role]
    out["a.only_test_decides"] = np.asarray(ONLY_TEST_DECIDES, dtype=np.int64)
    return {"normalize_golden.npz": out, "normalize_web30k.json": settings}


def main():
    for f, d in build().items():
        path = os.path.join(HERE, f)
        if f.endswith(".json"):
            with open(path, "w") as fh:
                json.dump(d, fh, indent=1)
                fh.write("\n")
        else:
            np.savez_compressed(path, **d)
        print(f, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
