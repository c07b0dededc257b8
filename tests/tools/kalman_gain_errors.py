"""The backward errors behind MARGIN of tests/test_gpu_kalman_gain.py, measured on an MI355X (not a test, not a gate):
python tests/tools/kalman_gain_errors.py [out.jsonl]

One JSON line per case of error_cases() there — dense random SPD systems through ebm_spd_solve_device, gains after real steps
through ebm_kalman_gain_device — with eta = ||x S - b||inf / (||S||inf ||x||inf + ||b||inf), evaluated in np.longdouble, of the
device and of numpy.linalg.solve on the same S and B (the largest over the right-hand sides), and the largest per-row ratio
eta_dev / max(eta_lapack, 2^-53).  A last line holds the largest ratio of all: MARGIN is four times it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as graft  # noqa: E402


def main():
    from test_gpu_kalman_gain import error_cases, error_ratios
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    worst = 0.0

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
    for label, S, B, X in error_cases(pkg):
        eta, eta_np, ratio = error_ratios(S, B, X)
        worst = max(worst, ratio)
        emit(dict(case=label, m=int(S.shape[0]), nrhs=int(B.shape[0]), eta_device=float(eta.max()), eta_lapack=float(eta_np.max()),
                  ratio=ratio, eta_device_over_m_eps=float(eta.max() / (S.shape[0] * 2.0 ** -53))))
    emit(dict(largest_ratio=worst, margin=4.0 * worst))


if __name__ == "__main__":
    main()
