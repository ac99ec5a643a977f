"""Which units go to which launch of the lane kernel (rsem_amd/csrc/unit_groups.hpp), without a GPU: tests/unit_groups_check.cpp
enumerates every small unit table (0..6 units, every compact <= main <= all, far queue / split_overlap / split rows / second
stream on and off) under the three EM loops and checks the plan against the launches written down loop by loop, that the launches
are disjoint, non-empty and cover every unit once, that nothing goes to a stream that does not exist, that the one-launch loop
always has a launch to carry its closers, the named groupings of tests/test_em_units_gpu.py launch by launch, and the two rules of
partition_units: which units are queued, and that the far group is adopted from one main unit in 25."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_of_every_small_unit_table(tmp_path):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("needs hipcc")
    exe = os.path.join(str(tmp_path), "unit_groups_check")
    # host compilation: the header holds no HIP
    subprocess.check_call([cc, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "unit_groups_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    n_cases, n_failed = int(p.stdout.split()[0]), int(p.stdout.split()[2])
    assert n_failed == 0 and n_cases > 1000
