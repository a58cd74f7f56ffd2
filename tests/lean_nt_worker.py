"""The child of tests/test_gpu_lean_ref.py::test_non_temporal_stores_bitwise (not a test module):
started with SMPQ_NT_MIN_MB=0 in its environment, so that every limb-plane output of this process is
stored with the non-temporal policy, it runs lean_ref.nt_cases (guarded, checked against the
reference) and saves the outputs.

    python tests/lean_nt_worker.py OUT.pt
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main(out_path):
    assert os.environ.get("SMPQ_NT_MIN_MB") == "0", "start me with SMPQ_NT_MIN_MB=0"
    import __graft_entry__
    __graft_entry__.build()
    import lean_ref
    torch.save(lean_ref.nt_cases(torch.device("cuda:0"), family="non-temporal stores"), out_path)


if __name__ == "__main__":
    main(sys.argv[1])
