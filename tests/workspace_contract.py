"""The four checks of a driver's caller-owned workspace (`void* workspace, size_t bytes`, or a scratch sized by a *_scratch_bytes
function) -- a plain helper module shared by tests/test_guardband_cpu.py (fake drivers on CPU tensors: the checks reject the wrong ones)
and tests/test_gpu_workspace_contract.py (the library's entry points).

A *family* is an object with
    inputs(shape, variant)        variant 0: the inputs under test; 1: other inputs of the same shape, for the dirtying call
    stages                        a list of functions stage(env, shape, inp, state): the entry point, or a forward / backward pair that
                                  communicates through the workspace; each asks env.ws(nbytes, tag) for every workspace it passes on and
                                  env.empty(...) for every output, and leaves its outputs in the dict `state`
    check(shape, inp, state)      compares the outputs with the family's oracle (variant 0 only)
    refused(exception)            whether a stage's exception is the S2VT_E_WORKSPACE refusal
    unused(shape)                 optional: the tags of scratch buffers the header documents as unused in this form of the call (per-step
                                  launches of a recurrence); check D then requires that the short buffer is accepted and never written
    refusal_checks_new_outputs    optional, False: a stage fills part of an output itself before it calls the driver (the histories' slot 0),
                                  so check D looks at the windows and at earlier stages' outputs only
`env` is a Provider: it owns one GuardedWorkspace per tag and decides how many of its bytes a stage is handed.

    A  exact_and_dirty   windows of exactly the declared size; a dirtying call, then the call under test on the same windows
    B  shrink            windows sized and dirtied by a larger shape; the smaller shape runs on them with the LARGER byte count
    C  containment       as B, but the smaller shape is given its own exact byte count: bytes [own, large) keep the snapshot's bits
    D  refusal           each stage in turn is handed declared - 256 bytes: it must refuse (family.refused(exception)), and neither a
                         window nor an output may change

A alone cannot see a store past the declared end that stays inside the last region's rounding up to 256 bytes: the bytes it lands in
belong to the window.  C can: there the declared end lies inside a larger window whose bytes behind it are compared with a snapshot."""
import torch

from guardband import SENTINEL16, SENTINEL32, SENTINEL64, GuardedWorkspace

_FILL = {1: (torch.uint8, 0xA5), 2: (torch.int16, SENTINEL16), 4: (torch.int32, SENTINEL32), 8: (torch.int64, SENTINEL64)}


def _sentinel_fill(t):
    itype, s = _FILL[t.element_size()]
    t.view(itype).fill_(s)
    return t


def _holds_sentinel(t):
    itype, s = _FILL[t.element_size()]
    return bool((t.view(itype) == s).all())


class Provider:
    """mode "exact": a window of exactly the bytes asked for (created on first use; a later request under the same tag must ask for the
    same size).  "whole": the existing (larger) window, all of it.  "own": the first nbytes of the existing window.  `short` = a set of
    tags (or True: every tag) that get 256 bytes less than they ask for."""

    def __init__(self, device):
        self.device, self.mode, self.short = device, "exact", ()
        self.windows, self.asked, self.made, self.log, self.regrown = {}, {}, [], [], set()
        self.stage = None

    def ws(self, nbytes, tag="default"):
        nbytes = int(nbytes)
        assert nbytes > 0, f"{tag}: the size function returned {nbytes}"
        self.asked[tag] = nbytes
        self.log.append((self.stage, tag))
        g = self.windows.get(tag)
        if g is None:
            g = self.windows[tag] = GuardedWorkspace(nbytes, device=self.device, name=tag)
        if self.mode == "exact":
            assert g.nbytes == nbytes, f"{tag}: {nbytes} bytes asked, the window has {g.nbytes}"
        elif nbytes > g.nbytes:
            # a size function need not grow with the shape (fewer rows may take a form that carves more): a grow-only cache then allocates
            # anew, from memory that earlier calls have used.  The new window holds the old one's stale bytes, repeated to its length.
            old, g = g, GuardedWorkspace(nbytes, device=self.device, name=tag)
            g.window.copy_(old.window.repeat(-(-nbytes // old.nbytes))[:nbytes])
            self.windows[tag] = g
            self.regrown.add(tag)
        give = g.nbytes if self.mode == "whole" else nbytes
        if self.short is True or tag in self.short:
            give = nbytes - 256
        return g.as_uint8(give)

    def empty(self, *size, dtype=torch.float32, **kw):
        """An output: sentinel bits everywhere, so that an element the call does not write is seen, and remembered for the refusal check."""
        kw.pop("device", None)
        t = _sentinel_fill(torch.empty(*size, dtype=dtype, device=self.device, **kw))
        self.made.append(t)
        return t

    def assert_intact(self):
        for g in self.windows.values():
            g.assert_intact()

    def sync(self):
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()


def _run(fam, env, shape, inp, upto=None):
    state = {}
    for i, stage in enumerate(fam.stages[:upto]):
        env.stage = i
        stage(env, shape, inp, state)
    env.sync()
    return state


def exact_and_dirty(fam, shape, device):
    env = Provider(device)
    _run(fam, env, shape, fam.inputs(shape, 1))
    env.assert_intact()
    inp = fam.inputs(shape, 0)
    state = _run(fam, env, shape, inp)
    env.assert_intact()
    fam.check(shape, inp, state)
    return env


def _dirtied_by_the_larger_shape(fam, large, device):
    env = Provider(device)
    _run(fam, env, large, fam.inputs(large, 1))
    env.assert_intact()
    return env


def shrink(fam, small, large, device):
    env = _dirtied_by_the_larger_shape(fam, large, device)
    env.mode = "whole"
    inp = fam.inputs(small, 0)
    state = _run(fam, env, small, inp)
    env.assert_intact()
    fam.check(small, inp, state)
    return env


def containment(fam, small, large, device, same_size_ok=False):
    env = _dirtied_by_the_larger_shape(fam, large, device)
    snaps = {tag: g.snapshot() for tag, g in env.windows.items()}
    env.mode, env.asked = "own", {}
    inp = fam.inputs(small, 0)
    state = _run(fam, env, small, inp)
    env.assert_intact()
    smaller = 0
    for tag, own in env.asked.items():
        g = env.windows[tag]
        if tag in env.regrown or tag not in snaps:                     # its own exact size: the guards are what lies behind it
            continue
        smaller += own < g.nbytes
        g.assert_unchanged(snaps[tag], own, g.nbytes, f"behind the {own} bytes declared for the smaller shape")
    assert smaller or env.regrown or same_size_ok, f"no workspace of {small} is smaller than that of {large}: the check compares nothing"
    fam.check(small, inp, state)
    return env


def refusal(fam, shape, device):
    """Stage by stage, tag by tag: the stages before it run as they should, then stage i gets one workspace 256 bytes short."""
    env = Provider(device)
    _run(fam, env, shape, fam.inputs(shape, 1))
    per_stage = {}
    for i, tag in env.log:
        per_stage.setdefault(i, [])
        if tag not in per_stage[i]:
            per_stage[i].append(tag)
    assert per_stage, "the family asked for no workspace"
    inp = fam.inputs(shape, 0)
    unused = fam.unused(shape) if hasattr(fam, "unused") else ()
    for i, tags in sorted(per_stage.items()):
        for tag in tags:
            env.short, env.made = (), []
            state = _run(fam, env, shape, inp, upto=i)
            snaps = {t: g.snapshot() for t, g in env.windows.items()}
            outs = [(t, t.clone()) for t in env.made]
            env.made, env.short, env.stage = [], {tag}, i
            if tag in unused:                                          # documented as unused in this form: accepted, and never touched
                fam.stages[i](env, shape, inp, state)
                env.sync()
                env.windows[tag].assert_unchanged(snaps[tag], 0, env.windows[tag].nbytes, f"stage {i}: {tag} is documented as unused in this form")
                env.assert_intact()
                continue
            try:
                fam.stages[i](env, shape, inp, state)
            except Exception as e:                                     # noqa: BLE001 -- the family says whether this is the refusal
                assert fam.refused(e), f"stage {i}, {tag} 256 bytes short: {e!r} is not the S2VT_E_WORKSPACE refusal"
            else:
                raise AssertionError(f"stage {i} accepted {tag} with {env.asked[tag] - 256} of {env.asked[tag]} bytes")
            env.sync()
            for t, g in env.windows.items():
                g.assert_unchanged(snaps[t], 0, g.nbytes, f"after stage {i} refused {tag}")
            env.assert_intact()
            for t, before in outs:
                assert torch.equal(t.view(torch.uint8), before.view(torch.uint8)), f"stage {i} refused {tag} and changed an earlier stage's output"
            for t in env.made if getattr(fam, "refusal_checks_new_outputs", True) else ():
                assert _holds_sentinel(t), f"stage {i} refused {tag} and wrote an output of shape {tuple(t.shape)}"
    env.short = ()
    return env
