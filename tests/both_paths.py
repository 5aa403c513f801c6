"""One script on one iteration path: the helper of the tests that compare the native iteration with the step-by-step one."""
import os
import subprocess
import sys
import tempfile

import numpy as np


def child(script, *args, no_native):
    """run `script` (python source; argv[1] the .npz it writes, then `args`) in a fresh process, with BDF_NO_NATIVE set or
    unset, and return what it saved"""
    env = {k: v for k, v in os.environ.items() if k != "BDF_NO_NATIVE"}
    if no_native:
        env["BDF_NO_NATIVE"] = "1"
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "o.npz")
        subprocess.run([sys.executable, "-W", "ignore", "-c", script, f, *[str(a) for a in args]], check=True, env=env, timeout=600)
        return dict(np.load(f))
