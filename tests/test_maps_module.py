"""Where the cohort map passes live: igcn_amd.maps, which stands on its own; igcn_amd.train re-exports the four names."""
import subprocess
import sys

from conftest import ROOT

PASSES = ("attention_maps", "association_maps", "connectivity_maps", "saliency_maps")


def test_train_reexports_the_passes_of_maps():
    from igcn_amd import maps, train
    for name in PASSES:
        assert getattr(train, name) is getattr(maps, name), name


def test_maps_imports_alone_in_a_fresh_interpreter():
    code = ("import sys, igcn_amd.maps as m; assert 'igcn_amd.train' not in sys.modules; "
            f"assert all(callable(getattr(m, n)) for n in {PASSES!r})")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
