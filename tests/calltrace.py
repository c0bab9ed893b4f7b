"""Record which libigcn entry points a piece of host code launches, in order (the way tools/trace_calls.py does), so a
test of an A/B switch can show that flipping it changed the path and not only that the numbers agree."""


def record_calls(monkeypatch):
    """Patch ``_lib.call`` (and the modules' imported names of it); return the list every call appends to: the entry
    point's name with its small integer and NULL arguments (device pointers and floats read as "*")."""
    from igcn_amd import _lib, ops, train
    orig, seen = _lib.call, []

    def traced(name, *args):
        seen.append((name,) + tuple(a if a is None or (type(a) is int and abs(a) < (1 << 31)) else "*" for a in args))
        return orig(name, *args)

    for mod in (_lib, ops, train):
        monkeypatch.setattr(mod, "call", traced)
    return seen
