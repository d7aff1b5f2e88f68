"""The colour-profile parser under AddressSanitizer + UBSan (CPU build only; tools/run_fuzz.sh icc): a stand-alone program drives
ist_icc.cpp and the profile walks of the three decoders over seeded random and adversarial profiles, bare and inside JPEG / PNG / WebP
containers, each from a heap block of exactly its size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_parser_under_sanitizers(tmp_path):
    env = dict(os.environ, IST_FUZZ_BIN=str(tmp_path / "check_icc_host"))
    r = subprocess.run([os.path.join(ROOT, "tools", "run_fuzz.sh"), "icc", "1500", "5"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1500 profiles" in r.stdout and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    counts = dict(zip(("none", "identity", "convert", "unsupported"), (int(v) for v in __import__("re").findall(r"(\d+)[,)]", r.stdout))))
    assert counts["convert"] > 100 and counts["unsupported"] > 100 and counts["none"] > 100      # the generator reaches both sides of every rule
