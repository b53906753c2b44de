"""The environment -> default copy tuning mapping that scripts/copy_tune.sh
sweeps with (STARWAY_COPY_BLOCKS / STARWAY_NT_THRESHOLD /
STARWAY_COPY_UNROLL). The tuning is read once per process, so each
configuration gets a fresh child. `_copy_tuning()` never touches the GPU:
this runs on GPU-less hosts."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
VARS = ("STARWAY_COPY_BLOCKS", "STARWAY_NT_THRESHOLD", "STARWAY_COPY_UNROLL")

CHILD = (
    "import json, sys; sys.path.insert(0, sys.argv[1]); "
    "from starway_amd import _core; "
    "print('TUNING ' + json.dumps(_core._copy_tuning()))"
)


def _child_tuning(extra_env):
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update(extra_env)
    out = subprocess.run([sys.executable, "-c", CHILD, str(REPO)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-800:]
    line = [l for l in out.stdout.splitlines() if l.startswith("TUNING ")][0]
    return json.loads(line[len("TUNING "):])


@pytest.mark.parametrize(
    "env,expect",
    [
        ({"STARWAY_COPY_BLOCKS": "3", "STARWAY_NT_THRESHOLD": "4096",
          "STARWAY_COPY_UNROLL": "8"},
         {"block_cap": 3, "nt_threshold": 4096, "nt_unroll": 8}),
        ({}, {"block_cap": 8192, "nt_threshold": 64 << 20, "nt_unroll": 4}),
    ],
    ids=["all_set", "defaults"])
def test_copy_tuning_from_environment(env, expect):
    assert _child_tuning(env) == expect
