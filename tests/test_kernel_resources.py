"""CPU: the compiler's resource report of the update kernel's forms (tools/kernel_resources.py --check): every k_update_pivot instance
without scratch and without a VGPR spill, the primal + PSE + lazy + banded instance within 104 VGPRs and 112 bytes of LDS.  The kernel
holds these with an allocator hint and empty asm statements; an edit or a compiler that loses them shows here.  One device-only compile."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_forms_meet_their_resource_requirements():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--match", "k_update_pivot", "--check"],
                       capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("k_update_pivot<") == 14 and "requirements met" in p.stdout
