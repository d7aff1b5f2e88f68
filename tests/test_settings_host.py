"""The context's settings word under ThreadSanitizer (CPU build only; tools/run_fuzz.sh settings): a stand-alone program includes
imagestitching_amd/csrc/ist_settings.h alone - no HIP, nothing preloaded - and runs five setter threads, one per field, against four
reader threads.  Every snapshot holds a valid value in every field, every invalid set is refused and changes nothing, and the word
ends as the last valid value each setter wrote."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_settings_word_under_thread_sanitizer(tmp_path):
    env = dict(os.environ, IST_FUZZ_BIN=str(tmp_path / "check_settings_host"))
    r = subprocess.run([os.path.join(ROOT, "tools", "run_fuzz.sh"), "settings", "20000"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "20000 sets per field" in r.stdout and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
