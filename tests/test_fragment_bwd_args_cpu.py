"""The fused backward's eleven C entries as an argument table: what each one refuses, which refusal wins when two apply, and which
empty calls succeed without work.  No GPU: the pointers are a dummy non-NULL value that nothing dereferences, and every call here
ends on the host -- refused, or an empty case with nothing to fill (a call that reached HIP would return a positive HIP code,
which the table does not admit).

EXPECTED was recorded by running this table against the library of the commit before the entries were folded into one
launcher, not written from reading the code; the folded launcher has to return the same code for every row."""
import os

import pytest

PTR = 4096      # (16-byte aligned: the oriented form checks the alignment of quats / g_quats)
MAX_K = 256     # VOGE_MAX_K

_ISO = "records sigmas shared sigma_mode rays"
_TAIL = "occ B N nrows W K C Nattr ws ws_bytes g_verts g_sigmas g_attr stream"
_GEN = "rays attr idx cnt weight act len dsd rgb wsum bg thr g gs0 gs1 g_hitlen occ B N nrows W K C Nattr ws ws_bytes acc_is_zero g_verts"
ARGS = {      # the entries' parameters in order, by the names used below (include/voge_hip.h)
    "voge_fragment_shade_bwd_iso": f"{_ISO} attr idx cnt weight act len dsd rgb wsum bg thr g gs0 gs1 {_TAIL}",
    "voge_fragment_merge_bwd_iso": f"{_ISO} attr idx cnt weight act len dsd g gs0 gs1 g_wsum {_TAIL}",
    "voge_fragment_bwd_iso": f"{_ISO} idx cnt weight act len dsd g gs0 gs1 g_hitlen occ B N nrows W K ws ws_bytes g_verts g_sigmas stream",
    "voge_fragment_shade_bwd": "mus isigmas rays attr idx cnt weight act len dsd rgb wsum bg thr g gs0 gs1 occ P nrows W K C Nattr ws ws_bytes "
                               "g_verts g_sigmas g_attr stream",
    "voge_fragment_merge_bwd": "mus isigmas rays attr idx cnt weight act len dsd g gs0 gs1 g_wsum occ P nrows W K C Nattr ws ws_bytes "
                               "g_verts g_sigmas g_attr stream",
    "voge_fragment_bwd": "mus isigmas rays idx cnt weight act len dsd g gs0 gs1 g_hitlen occ P nrows W K ws ws_bytes g_verts g_sigmas stream",
    "voge_frame_shade_bwd_iso": f"{_ISO} attr idx cnt weight len rgb wsum bg thr g gs0 gs1 {_TAIL}",
    "voge_frame_merge_bwd_iso": f"{_ISO} attr idx cnt weight len g gs0 gs1 g_wsum wsum_fwd {_TAIL}",
    "voge_frame_depth_bwd_iso": f"{_ISO} idx cnt weight len depth wsum g gs0 g_sil normalize occ B N nrows W K ws ws_bytes g_verts g_sigmas stream",
    "voge_frame_bwd_gen": f"form records shared_verts shared_sigmas kind {_GEN} g_sigmas g_attr stream",
    "voge_frame_bwd_ori": f"form records scales quats shared_verts shared_sigmas sigma_mode {_GEN} g_sigmas g_quats g_attr stream",
}
SCALARS = dict(shared=0, shared_verts=0, shared_sigmas=0, sigma_mode=1, form=0, kind=2, thr=-1.0, gs0=3, gs1=1, occ=1.0, B=2, N=50,
               P=100, nrows=14, W=10, K=5, C=3, Nattr=100, normalize=1, acc_is_zero=0, stream=None)
BYTES_PER_GAUSSIAN = {      # what each entry asks of its workspace / accumulator for the base call's 100 Gaussians
    "voge_fragment_shade_bwd_iso": 32, "voge_fragment_merge_bwd_iso": 32, "voge_fragment_bwd_iso": 16, "voge_fragment_shade_bwd": 112,
    "voge_fragment_merge_bwd": 112, "voge_fragment_bwd": 112, "voge_frame_shade_bwd_iso": 32, "voge_frame_merge_bwd_iso": 32,
    "voge_frame_depth_bwd_iso": 16, "voge_frame_bwd_gen": 64, "voge_frame_bwd_ori": 64}
# the pointers an entry insists on once there is work to do (the others may be NULL in some form of the call)
REQUIRED = {
    "voge_fragment_shade_bwd_iso": "records rays attr idx cnt weight len rgb wsum bg g ws",
    "voge_fragment_merge_bwd_iso": "records rays attr idx cnt weight len g ws",
    "voge_fragment_bwd_iso": "records rays idx cnt weight len ws g_verts g_sigmas",
    "voge_fragment_shade_bwd": "mus isigmas rays attr idx cnt weight len rgb wsum bg g ws",
    "voge_fragment_merge_bwd": "mus isigmas rays attr idx cnt weight len g ws",
    "voge_fragment_bwd": "mus isigmas rays idx cnt weight len ws g_verts g_sigmas",
    "voge_frame_shade_bwd_iso": "records rays attr idx cnt weight len rgb wsum bg g ws",
    "voge_frame_merge_bwd_iso": "records rays attr idx cnt weight len g ws",
    "voge_frame_depth_bwd_iso": "records rays idx cnt weight len depth wsum ws g_verts g_sigmas",
    "voge_frame_bwd_gen": "records rays attr idx cnt weight len rgb wsum bg g ws",
    "voge_frame_bwd_ori": "records scales quats rays attr idx cnt weight len rgb wsum bg g ws",
}
OUTPUTS = ("g_verts", "g_sigmas", "g_quats", "g_attr")


def base(entry):
    """A call that would run: every pointer given, a workspace of exactly the bytes the entry asks for."""
    names = ARGS[entry].split()
    call = {n: SCALARS.get(n, PTR) for n in names}
    call["ws_bytes"] = 100 * BYTES_PER_GAUSSIAN[entry]
    return call


def cases():
    """[(id, entry, overrides of base(entry))]: every row ends on the host."""
    out = []
    for entry in ARGS:
        names = ARGS[entry].split()
        b = base(entry)
        short = {"ws_bytes": b["ws_bytes"] - 1}
        iso = "B" in names
        weights = entry in ("voge_fragment_bwd_iso", "voge_fragment_bwd")
        gen = entry in ("voge_frame_bwd_gen", "voge_frame_bwd_ori")
        cap = MAX_K if weights else 128

        def add(what, **over):
            out.append((f"{entry[5:]}:{what}", entry, over))

        for n in ("B", "N", "P", "nrows", "W", "Nattr"):
            if n in names:
                add(f"{n}=-1", **{n: -1})
        add("K=0", K=0)
        add("K=-1", K=-1)
        if entry == "voge_frame_depth_bwd_iso":
            add("gs0=-1", gs0=-1)
        if "C" in names:
            add("C=0", C=0)
            add("C=5", C=5)
        if "sigma_mode" in names:
            for v in (-1, 0, 3):
                if v != 0 or entry == "voge_frame_bwd_ori":
                    add(f"sigma_mode={v}", sigma_mode=v)
        if gen:
            add("form=-1", form=-1)
            add("form=3", form=3)
            add("form=2,C=0,short", form=2, C=0, ws_bytes=100 * 48 - 1)      # (the weights' form takes no C)
            add("form=2,K=cap+1", form=2, K=MAX_K + 1)
            add("form=2,K=129,short", form=2, K=129, ws_bytes=100 * 48 - 1)
        if entry == "voge_frame_bwd_gen":
            add("kind=0", kind=0)
            add("kind=3", kind=3)
            add("kind=1,act,dsd", kind=1)
            add("kind=1,act,dsd,short", kind=1, ws_bytes=100 * 48 - 1)
            add("kind=1,short", kind=1, act=None, dsd=None, ws_bytes=100 * 48 - 1)
            add("kind=1,form=2,short", kind=1, form=2, act=None, dsd=None, ws_bytes=100 * 32 - 1)
            add("kind=1,form=2,K=129,short", kind=1, form=2, K=129, act=None, dsd=None, ws_bytes=100 * 32 - 1)
        add("K=cap+1", K=cap + 1)
        add("K=cap+1,short", K=cap + 1, **short)
        add("K=cap,short", K=cap, **short)
        for n in names:      # every pointer NULL in turn, the workspace short: -1 where the pointer is required, -2 where not
            if b[n] == PTR:
                add(f"{n}=NULL,short", **{n: None}, **short)
        for n in REQUIRED[entry].split():
            add(f"{n}=NULL", **{n: None})
        if "act" in names:
            add("act,no dsd", dsd=None)
            add("dsd,no act", act=None)
            add("act,no dsd,short", dsd=None, **short)
        if not weights and entry != "voge_frame_depth_bwd_iso":
            add("g_verts,no g_sigmas", g_sigmas=None)
            add("g_sigmas,no g_verts", g_verts=None)
            add("neither g_verts nor g_sigmas,short", g_verts=None, g_sigmas=None, **short)
        if "sigmas" in names:
            add("sigma_mode=2,no sigmas", sigma_mode=2, sigmas=None)
            add("sigma_mode=2,no sigmas,short", sigma_mode=2, sigmas=None, **short)
            add("sigma_mode=2,short", sigma_mode=2, **short)
            if not weights and entry != "voge_frame_depth_bwd_iso":
                add("sigma_mode=2,no sigmas,no gradients,short", sigma_mode=2, sigmas=None, g_verts=None, g_sigmas=None, **short)
        if entry == "voge_frame_depth_bwd_iso":
            add("neither g_depth nor g_sil", g=None, g_sil=None)
            add("g_sil only,short", g=None, **short)
        if entry == "voge_frame_bwd_ori":
            add("g_scales,no g_quats", g_quats=None)
            add("g_quats,no g_scales", g_sigmas=None)
            add("quats off 16 bytes", quats=PTR + 4)
            add("g_quats off 16 bytes", g_quats=PTR + 8)
            add("quats off 16 bytes,short", quats=PTR + 4, **short)
            add("quats off 16 bytes,no gradients,short", quats=PTR + 4, g_verts=None, g_sigmas=None, g_quats=None, **short)
            add("no scales,no gradients,short", scales=None, g_verts=None, g_sigmas=None, g_quats=None, **short)
            add("quats off 16 bytes,P=0", quats=PTR + 4, B=0, **{n: None for n in ("g_verts", "g_attr")})
        add("short", **short)
        big = {"B": 1, "N": 1 << 26} if iso else {"P": 1 << 26}
        add("P=2^26", ws_bytes=(1 << 26) * BYTES_PER_GAUSSIAN[entry], **big)
        add("P=2^26,short", ws_bytes=(1 << 26) * BYTES_PER_GAUSSIAN[entry] - 1, **big)
        if "Nattr" in names:
            add("Nattr*C=2^30", Nattr=1 << 28, C=4)
            add("Nattr*C=2^30,C=1", Nattr=1 << 30, C=1)
            add("Nattr*C=2^30,short", Nattr=1 << 28, C=4, **short)
            if gen:
                add("form=2,Nattr*C=2^30,short", form=2, Nattr=1 << 28, C=4, ws_bytes=100 * 48 - 1)
        # the empty cases: no output to fill, so nothing reaches HIP
        no_out = {n: None for n in OUTPUTS if n in names}
        none = {n: None for n in names if b[n] == PTR}
        for what, over in (("P=0", {"B": 0} if iso else {"P": 0}), ("N=0", {"N": 0}), ("B=0,N=0", {"B": 0, "N": 0}),
                           ("nrows=0", {"nrows": 0}), ("W=0", {"W": 0})):
            if all(n in names for n in over):
                add(f"{what},no outputs", **over, **no_out)
                add(f"{what},no pointers,short", **over, **none, ws_bytes=0)
                add(f"{what},K=cap+1", **over, **no_out, K=cap + 1)
        if "shared" in names:
            if weights or entry == "voge_frame_depth_bwd_iso":      # (no Gaussian to write to: the outputs are not looked at)
                add("shared,N=0", shared=1, N=0)
            add("shared,B=0,no outputs", shared=1, B=0, **no_out)
    return out


EXPECTED = {
    'fragment_shade_bwd_iso:B=-1': -1, 'fragment_shade_bwd_iso:N=-1': -1, 'fragment_shade_bwd_iso:nrows=-1': -1,
    'fragment_shade_bwd_iso:W=-1': -1, 'fragment_shade_bwd_iso:Nattr=-1': -1, 'fragment_shade_bwd_iso:K=0': -1,
    'fragment_shade_bwd_iso:K=-1': -1, 'fragment_shade_bwd_iso:C=0': -1, 'fragment_shade_bwd_iso:C=5': -1,
    'fragment_shade_bwd_iso:sigma_mode=-1': -1, 'fragment_shade_bwd_iso:sigma_mode=3': -1, 'fragment_shade_bwd_iso:K=cap+1': -3,
    'fragment_shade_bwd_iso:K=cap+1,short': -3, 'fragment_shade_bwd_iso:K=cap,short': -2,
    'fragment_shade_bwd_iso:records=NULL,short': -1, 'fragment_shade_bwd_iso:sigmas=NULL,short': -2,
    'fragment_shade_bwd_iso:rays=NULL,short': -1, 'fragment_shade_bwd_iso:attr=NULL,short': -1,
    'fragment_shade_bwd_iso:idx=NULL,short': -1, 'fragment_shade_bwd_iso:cnt=NULL,short': -1,
    'fragment_shade_bwd_iso:weight=NULL,short': -1, 'fragment_shade_bwd_iso:act=NULL,short': -1,
    'fragment_shade_bwd_iso:len=NULL,short': -1, 'fragment_shade_bwd_iso:dsd=NULL,short': -1,
    'fragment_shade_bwd_iso:rgb=NULL,short': -1, 'fragment_shade_bwd_iso:wsum=NULL,short': -1,
    'fragment_shade_bwd_iso:bg=NULL,short': -1, 'fragment_shade_bwd_iso:g=NULL,short': -1, 'fragment_shade_bwd_iso:ws=NULL,short': -1,
    'fragment_shade_bwd_iso:g_verts=NULL,short': -1, 'fragment_shade_bwd_iso:g_sigmas=NULL,short': -1,
    'fragment_shade_bwd_iso:g_attr=NULL,short': -2, 'fragment_shade_bwd_iso:records=NULL': -1, 'fragment_shade_bwd_iso:rays=NULL': -1,
    'fragment_shade_bwd_iso:attr=NULL': -1, 'fragment_shade_bwd_iso:idx=NULL': -1, 'fragment_shade_bwd_iso:cnt=NULL': -1,
    'fragment_shade_bwd_iso:weight=NULL': -1, 'fragment_shade_bwd_iso:len=NULL': -1, 'fragment_shade_bwd_iso:rgb=NULL': -1,
    'fragment_shade_bwd_iso:wsum=NULL': -1, 'fragment_shade_bwd_iso:bg=NULL': -1, 'fragment_shade_bwd_iso:g=NULL': -1,
    'fragment_shade_bwd_iso:ws=NULL': -1, 'fragment_shade_bwd_iso:act,no dsd': -1, 'fragment_shade_bwd_iso:dsd,no act': -1,
    'fragment_shade_bwd_iso:act,no dsd,short': -1, 'fragment_shade_bwd_iso:g_verts,no g_sigmas': -1,
    'fragment_shade_bwd_iso:g_sigmas,no g_verts': -1, 'fragment_shade_bwd_iso:neither g_verts nor g_sigmas,short': -2,
    'fragment_shade_bwd_iso:sigma_mode=2,no sigmas': -1, 'fragment_shade_bwd_iso:sigma_mode=2,no sigmas,short': -1,
    'fragment_shade_bwd_iso:sigma_mode=2,short': -2, 'fragment_shade_bwd_iso:sigma_mode=2,no sigmas,no gradients,short': -2,
    'fragment_shade_bwd_iso:short': -2, 'fragment_shade_bwd_iso:P=2^26': -1, 'fragment_shade_bwd_iso:P=2^26,short': -2,
    'fragment_shade_bwd_iso:Nattr*C=2^30': -1, 'fragment_shade_bwd_iso:Nattr*C=2^30,C=1': -1,
    'fragment_shade_bwd_iso:Nattr*C=2^30,short': -2, 'fragment_shade_bwd_iso:P=0,no outputs': 0,
    'fragment_shade_bwd_iso:P=0,no pointers,short': 0, 'fragment_shade_bwd_iso:P=0,K=cap+1': -3,
    'fragment_shade_bwd_iso:N=0,no outputs': 0, 'fragment_shade_bwd_iso:N=0,no pointers,short': 0,
    'fragment_shade_bwd_iso:N=0,K=cap+1': -3, 'fragment_shade_bwd_iso:B=0,N=0,no outputs': 0,
    'fragment_shade_bwd_iso:B=0,N=0,no pointers,short': 0, 'fragment_shade_bwd_iso:B=0,N=0,K=cap+1': -3,
    'fragment_shade_bwd_iso:nrows=0,no outputs': 0, 'fragment_shade_bwd_iso:nrows=0,no pointers,short': 0,
    'fragment_shade_bwd_iso:nrows=0,K=cap+1': -3, 'fragment_shade_bwd_iso:W=0,no outputs': 0,
    'fragment_shade_bwd_iso:W=0,no pointers,short': 0, 'fragment_shade_bwd_iso:W=0,K=cap+1': -3,
    'fragment_shade_bwd_iso:shared,B=0,no outputs': 0, 'fragment_merge_bwd_iso:B=-1': -1, 'fragment_merge_bwd_iso:N=-1': -1,
    'fragment_merge_bwd_iso:nrows=-1': -1, 'fragment_merge_bwd_iso:W=-1': -1, 'fragment_merge_bwd_iso:Nattr=-1': -1,
    'fragment_merge_bwd_iso:K=0': -1, 'fragment_merge_bwd_iso:K=-1': -1, 'fragment_merge_bwd_iso:C=0': -1,
    'fragment_merge_bwd_iso:C=5': -1, 'fragment_merge_bwd_iso:sigma_mode=-1': -1, 'fragment_merge_bwd_iso:sigma_mode=3': -1,
    'fragment_merge_bwd_iso:K=cap+1': -3, 'fragment_merge_bwd_iso:K=cap+1,short': -3, 'fragment_merge_bwd_iso:K=cap,short': -2,
    'fragment_merge_bwd_iso:records=NULL,short': -1, 'fragment_merge_bwd_iso:sigmas=NULL,short': -2,
    'fragment_merge_bwd_iso:rays=NULL,short': -1, 'fragment_merge_bwd_iso:attr=NULL,short': -1,
    'fragment_merge_bwd_iso:idx=NULL,short': -1, 'fragment_merge_bwd_iso:cnt=NULL,short': -1,
    'fragment_merge_bwd_iso:weight=NULL,short': -1, 'fragment_merge_bwd_iso:act=NULL,short': -1,
    'fragment_merge_bwd_iso:len=NULL,short': -1, 'fragment_merge_bwd_iso:dsd=NULL,short': -1, 'fragment_merge_bwd_iso:g=NULL,short': -1,
    'fragment_merge_bwd_iso:g_wsum=NULL,short': -2, 'fragment_merge_bwd_iso:ws=NULL,short': -1,
    'fragment_merge_bwd_iso:g_verts=NULL,short': -1, 'fragment_merge_bwd_iso:g_sigmas=NULL,short': -1,
    'fragment_merge_bwd_iso:g_attr=NULL,short': -2, 'fragment_merge_bwd_iso:records=NULL': -1, 'fragment_merge_bwd_iso:rays=NULL': -1,
    'fragment_merge_bwd_iso:attr=NULL': -1, 'fragment_merge_bwd_iso:idx=NULL': -1, 'fragment_merge_bwd_iso:cnt=NULL': -1,
    'fragment_merge_bwd_iso:weight=NULL': -1, 'fragment_merge_bwd_iso:len=NULL': -1, 'fragment_merge_bwd_iso:g=NULL': -1,
    'fragment_merge_bwd_iso:ws=NULL': -1, 'fragment_merge_bwd_iso:act,no dsd': -1, 'fragment_merge_bwd_iso:dsd,no act': -1,
    'fragment_merge_bwd_iso:act,no dsd,short': -1, 'fragment_merge_bwd_iso:g_verts,no g_sigmas': -1,
    'fragment_merge_bwd_iso:g_sigmas,no g_verts': -1, 'fragment_merge_bwd_iso:neither g_verts nor g_sigmas,short': -2,
    'fragment_merge_bwd_iso:sigma_mode=2,no sigmas': -1, 'fragment_merge_bwd_iso:sigma_mode=2,no sigmas,short': -1,
    'fragment_merge_bwd_iso:sigma_mode=2,short': -2, 'fragment_merge_bwd_iso:sigma_mode=2,no sigmas,no gradients,short': -2,
    'fragment_merge_bwd_iso:short': -2, 'fragment_merge_bwd_iso:P=2^26': -1, 'fragment_merge_bwd_iso:P=2^26,short': -2,
    'fragment_merge_bwd_iso:Nattr*C=2^30': -1, 'fragment_merge_bwd_iso:Nattr*C=2^30,C=1': -1,
    'fragment_merge_bwd_iso:Nattr*C=2^30,short': -2, 'fragment_merge_bwd_iso:P=0,no outputs': 0,
    'fragment_merge_bwd_iso:P=0,no pointers,short': 0, 'fragment_merge_bwd_iso:P=0,K=cap+1': -3,
    'fragment_merge_bwd_iso:N=0,no outputs': 0, 'fragment_merge_bwd_iso:N=0,no pointers,short': 0,
    'fragment_merge_bwd_iso:N=0,K=cap+1': -3, 'fragment_merge_bwd_iso:B=0,N=0,no outputs': 0,
    'fragment_merge_bwd_iso:B=0,N=0,no pointers,short': 0, 'fragment_merge_bwd_iso:B=0,N=0,K=cap+1': -3,
    'fragment_merge_bwd_iso:nrows=0,no outputs': 0, 'fragment_merge_bwd_iso:nrows=0,no pointers,short': 0,
    'fragment_merge_bwd_iso:nrows=0,K=cap+1': -3, 'fragment_merge_bwd_iso:W=0,no outputs': 0,
    'fragment_merge_bwd_iso:W=0,no pointers,short': 0, 'fragment_merge_bwd_iso:W=0,K=cap+1': -3,
    'fragment_merge_bwd_iso:shared,B=0,no outputs': 0, 'fragment_bwd_iso:B=-1': -1, 'fragment_bwd_iso:N=-1': -1,
    'fragment_bwd_iso:nrows=-1': -1, 'fragment_bwd_iso:W=-1': -1, 'fragment_bwd_iso:K=0': -1, 'fragment_bwd_iso:K=-1': -1,
    'fragment_bwd_iso:sigma_mode=-1': -1, 'fragment_bwd_iso:sigma_mode=3': -1, 'fragment_bwd_iso:K=cap+1': -3,
    'fragment_bwd_iso:K=cap+1,short': -3, 'fragment_bwd_iso:K=cap,short': -2, 'fragment_bwd_iso:records=NULL,short': -1,
    'fragment_bwd_iso:sigmas=NULL,short': -2, 'fragment_bwd_iso:rays=NULL,short': -1, 'fragment_bwd_iso:idx=NULL,short': -1,
    'fragment_bwd_iso:cnt=NULL,short': -1, 'fragment_bwd_iso:weight=NULL,short': -1, 'fragment_bwd_iso:act=NULL,short': -1,
    'fragment_bwd_iso:len=NULL,short': -1, 'fragment_bwd_iso:dsd=NULL,short': -1, 'fragment_bwd_iso:g=NULL,short': -2,
    'fragment_bwd_iso:g_hitlen=NULL,short': -2, 'fragment_bwd_iso:ws=NULL,short': -1, 'fragment_bwd_iso:g_verts=NULL,short': -1,
    'fragment_bwd_iso:g_sigmas=NULL,short': -1, 'fragment_bwd_iso:records=NULL': -1, 'fragment_bwd_iso:rays=NULL': -1,
    'fragment_bwd_iso:idx=NULL': -1, 'fragment_bwd_iso:cnt=NULL': -1, 'fragment_bwd_iso:weight=NULL': -1,
    'fragment_bwd_iso:len=NULL': -1, 'fragment_bwd_iso:ws=NULL': -1, 'fragment_bwd_iso:g_verts=NULL': -1,
    'fragment_bwd_iso:g_sigmas=NULL': -1, 'fragment_bwd_iso:act,no dsd': -1, 'fragment_bwd_iso:dsd,no act': -1,
    'fragment_bwd_iso:act,no dsd,short': -1, 'fragment_bwd_iso:sigma_mode=2,no sigmas': -1,
    'fragment_bwd_iso:sigma_mode=2,no sigmas,short': -1, 'fragment_bwd_iso:sigma_mode=2,short': -2, 'fragment_bwd_iso:short': -2,
    'fragment_bwd_iso:P=2^26': -1, 'fragment_bwd_iso:P=2^26,short': -2, 'fragment_bwd_iso:P=0,no outputs': 0,
    'fragment_bwd_iso:P=0,no pointers,short': 0, 'fragment_bwd_iso:P=0,K=cap+1': -3, 'fragment_bwd_iso:N=0,no outputs': 0,
    'fragment_bwd_iso:N=0,no pointers,short': 0, 'fragment_bwd_iso:N=0,K=cap+1': -3, 'fragment_bwd_iso:B=0,N=0,no outputs': 0,
    'fragment_bwd_iso:B=0,N=0,no pointers,short': 0, 'fragment_bwd_iso:B=0,N=0,K=cap+1': -3, 'fragment_bwd_iso:nrows=0,no outputs': -1,
    'fragment_bwd_iso:nrows=0,no pointers,short': -1, 'fragment_bwd_iso:nrows=0,K=cap+1': -3, 'fragment_bwd_iso:W=0,no outputs': -1,
    'fragment_bwd_iso:W=0,no pointers,short': -1, 'fragment_bwd_iso:W=0,K=cap+1': -3, 'fragment_bwd_iso:shared,N=0': 0,
    'fragment_bwd_iso:shared,B=0,no outputs': -1, 'fragment_shade_bwd:P=-1': -1, 'fragment_shade_bwd:nrows=-1': -1,
    'fragment_shade_bwd:W=-1': -1, 'fragment_shade_bwd:Nattr=-1': -1, 'fragment_shade_bwd:K=0': -1, 'fragment_shade_bwd:K=-1': -1,
    'fragment_shade_bwd:C=0': -1, 'fragment_shade_bwd:C=5': -1, 'fragment_shade_bwd:K=cap+1': -3, 'fragment_shade_bwd:K=cap+1,short': -3,
    'fragment_shade_bwd:K=cap,short': -2, 'fragment_shade_bwd:mus=NULL,short': -1, 'fragment_shade_bwd:isigmas=NULL,short': -1,
    'fragment_shade_bwd:rays=NULL,short': -1, 'fragment_shade_bwd:attr=NULL,short': -1, 'fragment_shade_bwd:idx=NULL,short': -1,
    'fragment_shade_bwd:cnt=NULL,short': -1, 'fragment_shade_bwd:weight=NULL,short': -1, 'fragment_shade_bwd:act=NULL,short': -1,
    'fragment_shade_bwd:len=NULL,short': -1, 'fragment_shade_bwd:dsd=NULL,short': -1, 'fragment_shade_bwd:rgb=NULL,short': -1,
    'fragment_shade_bwd:wsum=NULL,short': -1, 'fragment_shade_bwd:bg=NULL,short': -1, 'fragment_shade_bwd:g=NULL,short': -1,
    'fragment_shade_bwd:ws=NULL,short': -1, 'fragment_shade_bwd:g_verts=NULL,short': -1, 'fragment_shade_bwd:g_sigmas=NULL,short': -1,
    'fragment_shade_bwd:g_attr=NULL,short': -2, 'fragment_shade_bwd:mus=NULL': -1, 'fragment_shade_bwd:isigmas=NULL': -1,
    'fragment_shade_bwd:rays=NULL': -1, 'fragment_shade_bwd:attr=NULL': -1, 'fragment_shade_bwd:idx=NULL': -1,
    'fragment_shade_bwd:cnt=NULL': -1, 'fragment_shade_bwd:weight=NULL': -1, 'fragment_shade_bwd:len=NULL': -1,
    'fragment_shade_bwd:rgb=NULL': -1, 'fragment_shade_bwd:wsum=NULL': -1, 'fragment_shade_bwd:bg=NULL': -1,
    'fragment_shade_bwd:g=NULL': -1, 'fragment_shade_bwd:ws=NULL': -1, 'fragment_shade_bwd:act,no dsd': -1,
    'fragment_shade_bwd:dsd,no act': -1, 'fragment_shade_bwd:act,no dsd,short': -1, 'fragment_shade_bwd:g_verts,no g_sigmas': -1,
    'fragment_shade_bwd:g_sigmas,no g_verts': -1, 'fragment_shade_bwd:neither g_verts nor g_sigmas,short': -2,
    'fragment_shade_bwd:short': -2, 'fragment_shade_bwd:P=2^26': -1, 'fragment_shade_bwd:P=2^26,short': -2,
    'fragment_shade_bwd:Nattr*C=2^30': -1, 'fragment_shade_bwd:Nattr*C=2^30,C=1': -1, 'fragment_shade_bwd:Nattr*C=2^30,short': -2,
    'fragment_shade_bwd:P=0,no outputs': 0, 'fragment_shade_bwd:P=0,no pointers,short': 0, 'fragment_shade_bwd:P=0,K=cap+1': -3,
    'fragment_shade_bwd:nrows=0,no outputs': 0, 'fragment_shade_bwd:nrows=0,no pointers,short': 0,
    'fragment_shade_bwd:nrows=0,K=cap+1': -3, 'fragment_shade_bwd:W=0,no outputs': 0, 'fragment_shade_bwd:W=0,no pointers,short': 0,
    'fragment_shade_bwd:W=0,K=cap+1': -3, 'fragment_merge_bwd:P=-1': -1, 'fragment_merge_bwd:nrows=-1': -1,
    'fragment_merge_bwd:W=-1': -1, 'fragment_merge_bwd:Nattr=-1': -1, 'fragment_merge_bwd:K=0': -1, 'fragment_merge_bwd:K=-1': -1,
    'fragment_merge_bwd:C=0': -1, 'fragment_merge_bwd:C=5': -1, 'fragment_merge_bwd:K=cap+1': -3, 'fragment_merge_bwd:K=cap+1,short': -3,
    'fragment_merge_bwd:K=cap,short': -2, 'fragment_merge_bwd:mus=NULL,short': -1, 'fragment_merge_bwd:isigmas=NULL,short': -1,
    'fragment_merge_bwd:rays=NULL,short': -1, 'fragment_merge_bwd:attr=NULL,short': -1, 'fragment_merge_bwd:idx=NULL,short': -1,
    'fragment_merge_bwd:cnt=NULL,short': -1, 'fragment_merge_bwd:weight=NULL,short': -1, 'fragment_merge_bwd:act=NULL,short': -1,
    'fragment_merge_bwd:len=NULL,short': -1, 'fragment_merge_bwd:dsd=NULL,short': -1, 'fragment_merge_bwd:g=NULL,short': -1,
    'fragment_merge_bwd:g_wsum=NULL,short': -2, 'fragment_merge_bwd:ws=NULL,short': -1, 'fragment_merge_bwd:g_verts=NULL,short': -1,
    'fragment_merge_bwd:g_sigmas=NULL,short': -1, 'fragment_merge_bwd:g_attr=NULL,short': -2, 'fragment_merge_bwd:mus=NULL': -1,
    'fragment_merge_bwd:isigmas=NULL': -1, 'fragment_merge_bwd:rays=NULL': -1, 'fragment_merge_bwd:attr=NULL': -1,
    'fragment_merge_bwd:idx=NULL': -1, 'fragment_merge_bwd:cnt=NULL': -1, 'fragment_merge_bwd:weight=NULL': -1,
    'fragment_merge_bwd:len=NULL': -1, 'fragment_merge_bwd:g=NULL': -1, 'fragment_merge_bwd:ws=NULL': -1,
    'fragment_merge_bwd:act,no dsd': -1, 'fragment_merge_bwd:dsd,no act': -1, 'fragment_merge_bwd:act,no dsd,short': -1,
    'fragment_merge_bwd:g_verts,no g_sigmas': -1, 'fragment_merge_bwd:g_sigmas,no g_verts': -1,
    'fragment_merge_bwd:neither g_verts nor g_sigmas,short': -2, 'fragment_merge_bwd:short': -2, 'fragment_merge_bwd:P=2^26': -1,
    'fragment_merge_bwd:P=2^26,short': -2, 'fragment_merge_bwd:Nattr*C=2^30': -1, 'fragment_merge_bwd:Nattr*C=2^30,C=1': -1,
    'fragment_merge_bwd:Nattr*C=2^30,short': -2, 'fragment_merge_bwd:P=0,no outputs': 0, 'fragment_merge_bwd:P=0,no pointers,short': 0,
    'fragment_merge_bwd:P=0,K=cap+1': -3, 'fragment_merge_bwd:nrows=0,no outputs': 0, 'fragment_merge_bwd:nrows=0,no pointers,short': 0,
    'fragment_merge_bwd:nrows=0,K=cap+1': -3, 'fragment_merge_bwd:W=0,no outputs': 0, 'fragment_merge_bwd:W=0,no pointers,short': 0,
    'fragment_merge_bwd:W=0,K=cap+1': -3, 'fragment_bwd:P=-1': -1, 'fragment_bwd:nrows=-1': -1, 'fragment_bwd:W=-1': -1,
    'fragment_bwd:K=0': -1, 'fragment_bwd:K=-1': -1, 'fragment_bwd:K=cap+1': -3, 'fragment_bwd:K=cap+1,short': -3,
    'fragment_bwd:K=cap,short': -2, 'fragment_bwd:mus=NULL,short': -1, 'fragment_bwd:isigmas=NULL,short': -1,
    'fragment_bwd:rays=NULL,short': -1, 'fragment_bwd:idx=NULL,short': -1, 'fragment_bwd:cnt=NULL,short': -1,
    'fragment_bwd:weight=NULL,short': -1, 'fragment_bwd:act=NULL,short': -1, 'fragment_bwd:len=NULL,short': -1,
    'fragment_bwd:dsd=NULL,short': -1, 'fragment_bwd:g=NULL,short': -2, 'fragment_bwd:g_hitlen=NULL,short': -2,
    'fragment_bwd:ws=NULL,short': -1, 'fragment_bwd:g_verts=NULL,short': -1, 'fragment_bwd:g_sigmas=NULL,short': -1,
    'fragment_bwd:mus=NULL': -1, 'fragment_bwd:isigmas=NULL': -1, 'fragment_bwd:rays=NULL': -1, 'fragment_bwd:idx=NULL': -1,
    'fragment_bwd:cnt=NULL': -1, 'fragment_bwd:weight=NULL': -1, 'fragment_bwd:len=NULL': -1, 'fragment_bwd:ws=NULL': -1,
    'fragment_bwd:g_verts=NULL': -1, 'fragment_bwd:g_sigmas=NULL': -1, 'fragment_bwd:act,no dsd': -1, 'fragment_bwd:dsd,no act': -1,
    'fragment_bwd:act,no dsd,short': -1, 'fragment_bwd:short': -2, 'fragment_bwd:P=2^26': -1, 'fragment_bwd:P=2^26,short': -2,
    'fragment_bwd:P=0,no outputs': 0, 'fragment_bwd:P=0,no pointers,short': 0, 'fragment_bwd:P=0,K=cap+1': -3,
    'fragment_bwd:nrows=0,no outputs': -1, 'fragment_bwd:nrows=0,no pointers,short': -1, 'fragment_bwd:nrows=0,K=cap+1': -3,
    'fragment_bwd:W=0,no outputs': -1, 'fragment_bwd:W=0,no pointers,short': -1, 'fragment_bwd:W=0,K=cap+1': -3,
    'frame_shade_bwd_iso:B=-1': -1, 'frame_shade_bwd_iso:N=-1': -1, 'frame_shade_bwd_iso:nrows=-1': -1, 'frame_shade_bwd_iso:W=-1': -1,
    'frame_shade_bwd_iso:Nattr=-1': -1, 'frame_shade_bwd_iso:K=0': -1, 'frame_shade_bwd_iso:K=-1': -1, 'frame_shade_bwd_iso:C=0': -1,
    'frame_shade_bwd_iso:C=5': -1, 'frame_shade_bwd_iso:sigma_mode=-1': -1, 'frame_shade_bwd_iso:sigma_mode=3': -1,
    'frame_shade_bwd_iso:K=cap+1': -3, 'frame_shade_bwd_iso:K=cap+1,short': -3, 'frame_shade_bwd_iso:K=cap,short': -2,
    'frame_shade_bwd_iso:records=NULL,short': -1, 'frame_shade_bwd_iso:sigmas=NULL,short': -2, 'frame_shade_bwd_iso:rays=NULL,short': -1,
    'frame_shade_bwd_iso:attr=NULL,short': -1, 'frame_shade_bwd_iso:idx=NULL,short': -1, 'frame_shade_bwd_iso:cnt=NULL,short': -1,
    'frame_shade_bwd_iso:weight=NULL,short': -1, 'frame_shade_bwd_iso:len=NULL,short': -1, 'frame_shade_bwd_iso:rgb=NULL,short': -1,
    'frame_shade_bwd_iso:wsum=NULL,short': -1, 'frame_shade_bwd_iso:bg=NULL,short': -1, 'frame_shade_bwd_iso:g=NULL,short': -1,
    'frame_shade_bwd_iso:ws=NULL,short': -1, 'frame_shade_bwd_iso:g_verts=NULL,short': -1, 'frame_shade_bwd_iso:g_sigmas=NULL,short': -1,
    'frame_shade_bwd_iso:g_attr=NULL,short': -2, 'frame_shade_bwd_iso:records=NULL': -1, 'frame_shade_bwd_iso:rays=NULL': -1,
    'frame_shade_bwd_iso:attr=NULL': -1, 'frame_shade_bwd_iso:idx=NULL': -1, 'frame_shade_bwd_iso:cnt=NULL': -1,
    'frame_shade_bwd_iso:weight=NULL': -1, 'frame_shade_bwd_iso:len=NULL': -1, 'frame_shade_bwd_iso:rgb=NULL': -1,
    'frame_shade_bwd_iso:wsum=NULL': -1, 'frame_shade_bwd_iso:bg=NULL': -1, 'frame_shade_bwd_iso:g=NULL': -1,
    'frame_shade_bwd_iso:ws=NULL': -1, 'frame_shade_bwd_iso:g_verts,no g_sigmas': -1, 'frame_shade_bwd_iso:g_sigmas,no g_verts': -1,
    'frame_shade_bwd_iso:neither g_verts nor g_sigmas,short': -2, 'frame_shade_bwd_iso:sigma_mode=2,no sigmas': -1,
    'frame_shade_bwd_iso:sigma_mode=2,no sigmas,short': -1, 'frame_shade_bwd_iso:sigma_mode=2,short': -2,
    'frame_shade_bwd_iso:sigma_mode=2,no sigmas,no gradients,short': -2, 'frame_shade_bwd_iso:short': -2,
    'frame_shade_bwd_iso:P=2^26': -1, 'frame_shade_bwd_iso:P=2^26,short': -2, 'frame_shade_bwd_iso:Nattr*C=2^30': -1,
    'frame_shade_bwd_iso:Nattr*C=2^30,C=1': -1, 'frame_shade_bwd_iso:Nattr*C=2^30,short': -2, 'frame_shade_bwd_iso:P=0,no outputs': 0,
    'frame_shade_bwd_iso:P=0,no pointers,short': 0, 'frame_shade_bwd_iso:P=0,K=cap+1': -3, 'frame_shade_bwd_iso:N=0,no outputs': 0,
    'frame_shade_bwd_iso:N=0,no pointers,short': 0, 'frame_shade_bwd_iso:N=0,K=cap+1': -3, 'frame_shade_bwd_iso:B=0,N=0,no outputs': 0,
    'frame_shade_bwd_iso:B=0,N=0,no pointers,short': 0, 'frame_shade_bwd_iso:B=0,N=0,K=cap+1': -3,
    'frame_shade_bwd_iso:nrows=0,no outputs': 0, 'frame_shade_bwd_iso:nrows=0,no pointers,short': 0,
    'frame_shade_bwd_iso:nrows=0,K=cap+1': -3, 'frame_shade_bwd_iso:W=0,no outputs': 0, 'frame_shade_bwd_iso:W=0,no pointers,short': 0,
    'frame_shade_bwd_iso:W=0,K=cap+1': -3, 'frame_shade_bwd_iso:shared,B=0,no outputs': 0, 'frame_merge_bwd_iso:B=-1': -1,
    'frame_merge_bwd_iso:N=-1': -1, 'frame_merge_bwd_iso:nrows=-1': -1, 'frame_merge_bwd_iso:W=-1': -1,
    'frame_merge_bwd_iso:Nattr=-1': -1, 'frame_merge_bwd_iso:K=0': -1, 'frame_merge_bwd_iso:K=-1': -1, 'frame_merge_bwd_iso:C=0': -1,
    'frame_merge_bwd_iso:C=5': -1, 'frame_merge_bwd_iso:sigma_mode=-1': -1, 'frame_merge_bwd_iso:sigma_mode=3': -1,
    'frame_merge_bwd_iso:K=cap+1': -3, 'frame_merge_bwd_iso:K=cap+1,short': -3, 'frame_merge_bwd_iso:K=cap,short': -2,
    'frame_merge_bwd_iso:records=NULL,short': -1, 'frame_merge_bwd_iso:sigmas=NULL,short': -2, 'frame_merge_bwd_iso:rays=NULL,short': -1,
    'frame_merge_bwd_iso:attr=NULL,short': -1, 'frame_merge_bwd_iso:idx=NULL,short': -1, 'frame_merge_bwd_iso:cnt=NULL,short': -1,
    'frame_merge_bwd_iso:weight=NULL,short': -1, 'frame_merge_bwd_iso:len=NULL,short': -1, 'frame_merge_bwd_iso:g=NULL,short': -1,
    'frame_merge_bwd_iso:g_wsum=NULL,short': -2, 'frame_merge_bwd_iso:wsum_fwd=NULL,short': -2, 'frame_merge_bwd_iso:ws=NULL,short': -1,
    'frame_merge_bwd_iso:g_verts=NULL,short': -1, 'frame_merge_bwd_iso:g_sigmas=NULL,short': -1,
    'frame_merge_bwd_iso:g_attr=NULL,short': -2, 'frame_merge_bwd_iso:records=NULL': -1, 'frame_merge_bwd_iso:rays=NULL': -1,
    'frame_merge_bwd_iso:attr=NULL': -1, 'frame_merge_bwd_iso:idx=NULL': -1, 'frame_merge_bwd_iso:cnt=NULL': -1,
    'frame_merge_bwd_iso:weight=NULL': -1, 'frame_merge_bwd_iso:len=NULL': -1, 'frame_merge_bwd_iso:g=NULL': -1,
    'frame_merge_bwd_iso:ws=NULL': -1, 'frame_merge_bwd_iso:g_verts,no g_sigmas': -1, 'frame_merge_bwd_iso:g_sigmas,no g_verts': -1,
    'frame_merge_bwd_iso:neither g_verts nor g_sigmas,short': -2, 'frame_merge_bwd_iso:sigma_mode=2,no sigmas': -1,
    'frame_merge_bwd_iso:sigma_mode=2,no sigmas,short': -1, 'frame_merge_bwd_iso:sigma_mode=2,short': -2,
    'frame_merge_bwd_iso:sigma_mode=2,no sigmas,no gradients,short': -2, 'frame_merge_bwd_iso:short': -2,
    'frame_merge_bwd_iso:P=2^26': -1, 'frame_merge_bwd_iso:P=2^26,short': -2, 'frame_merge_bwd_iso:Nattr*C=2^30': -1,
    'frame_merge_bwd_iso:Nattr*C=2^30,C=1': -1, 'frame_merge_bwd_iso:Nattr*C=2^30,short': -2, 'frame_merge_bwd_iso:P=0,no outputs': 0,
    'frame_merge_bwd_iso:P=0,no pointers,short': 0, 'frame_merge_bwd_iso:P=0,K=cap+1': -3, 'frame_merge_bwd_iso:N=0,no outputs': 0,
    'frame_merge_bwd_iso:N=0,no pointers,short': 0, 'frame_merge_bwd_iso:N=0,K=cap+1': -3, 'frame_merge_bwd_iso:B=0,N=0,no outputs': 0,
    'frame_merge_bwd_iso:B=0,N=0,no pointers,short': 0, 'frame_merge_bwd_iso:B=0,N=0,K=cap+1': -3,
    'frame_merge_bwd_iso:nrows=0,no outputs': 0, 'frame_merge_bwd_iso:nrows=0,no pointers,short': 0,
    'frame_merge_bwd_iso:nrows=0,K=cap+1': -3, 'frame_merge_bwd_iso:W=0,no outputs': 0, 'frame_merge_bwd_iso:W=0,no pointers,short': 0,
    'frame_merge_bwd_iso:W=0,K=cap+1': -3, 'frame_merge_bwd_iso:shared,B=0,no outputs': 0, 'frame_depth_bwd_iso:B=-1': -1,
    'frame_depth_bwd_iso:N=-1': -1, 'frame_depth_bwd_iso:nrows=-1': -1, 'frame_depth_bwd_iso:W=-1': -1, 'frame_depth_bwd_iso:K=0': -1,
    'frame_depth_bwd_iso:K=-1': -1, 'frame_depth_bwd_iso:gs0=-1': -1, 'frame_depth_bwd_iso:sigma_mode=-1': -1,
    'frame_depth_bwd_iso:sigma_mode=3': -1, 'frame_depth_bwd_iso:K=cap+1': -3, 'frame_depth_bwd_iso:K=cap+1,short': -3,
    'frame_depth_bwd_iso:K=cap,short': -2, 'frame_depth_bwd_iso:records=NULL,short': -1, 'frame_depth_bwd_iso:sigmas=NULL,short': -2,
    'frame_depth_bwd_iso:rays=NULL,short': -1, 'frame_depth_bwd_iso:idx=NULL,short': -1, 'frame_depth_bwd_iso:cnt=NULL,short': -1,
    'frame_depth_bwd_iso:weight=NULL,short': -1, 'frame_depth_bwd_iso:len=NULL,short': -1, 'frame_depth_bwd_iso:depth=NULL,short': -1,
    'frame_depth_bwd_iso:wsum=NULL,short': -1, 'frame_depth_bwd_iso:g=NULL,short': -2, 'frame_depth_bwd_iso:g_sil=NULL,short': -2,
    'frame_depth_bwd_iso:ws=NULL,short': -1, 'frame_depth_bwd_iso:g_verts=NULL,short': -1, 'frame_depth_bwd_iso:g_sigmas=NULL,short': -1,
    'frame_depth_bwd_iso:records=NULL': -1, 'frame_depth_bwd_iso:rays=NULL': -1, 'frame_depth_bwd_iso:idx=NULL': -1,
    'frame_depth_bwd_iso:cnt=NULL': -1, 'frame_depth_bwd_iso:weight=NULL': -1, 'frame_depth_bwd_iso:len=NULL': -1,
    'frame_depth_bwd_iso:depth=NULL': -1, 'frame_depth_bwd_iso:wsum=NULL': -1, 'frame_depth_bwd_iso:ws=NULL': -1,
    'frame_depth_bwd_iso:g_verts=NULL': -1, 'frame_depth_bwd_iso:g_sigmas=NULL': -1, 'frame_depth_bwd_iso:sigma_mode=2,no sigmas': -1,
    'frame_depth_bwd_iso:sigma_mode=2,no sigmas,short': -1, 'frame_depth_bwd_iso:sigma_mode=2,short': -2,
    'frame_depth_bwd_iso:neither g_depth nor g_sil': -1, 'frame_depth_bwd_iso:g_sil only,short': -2, 'frame_depth_bwd_iso:short': -2,
    'frame_depth_bwd_iso:P=2^26': -1, 'frame_depth_bwd_iso:P=2^26,short': -2, 'frame_depth_bwd_iso:P=0,no outputs': 0,
    'frame_depth_bwd_iso:P=0,no pointers,short': 0, 'frame_depth_bwd_iso:P=0,K=cap+1': -3, 'frame_depth_bwd_iso:N=0,no outputs': 0,
    'frame_depth_bwd_iso:N=0,no pointers,short': 0, 'frame_depth_bwd_iso:N=0,K=cap+1': -3, 'frame_depth_bwd_iso:B=0,N=0,no outputs': 0,
    'frame_depth_bwd_iso:B=0,N=0,no pointers,short': 0, 'frame_depth_bwd_iso:B=0,N=0,K=cap+1': -3,
    'frame_depth_bwd_iso:nrows=0,no outputs': -1, 'frame_depth_bwd_iso:nrows=0,no pointers,short': -1,
    'frame_depth_bwd_iso:nrows=0,K=cap+1': -3, 'frame_depth_bwd_iso:W=0,no outputs': -1, 'frame_depth_bwd_iso:W=0,no pointers,short': -1,
    'frame_depth_bwd_iso:W=0,K=cap+1': -3, 'frame_depth_bwd_iso:shared,N=0': 0, 'frame_depth_bwd_iso:shared,B=0,no outputs': -1,
    'frame_bwd_gen:B=-1': -1, 'frame_bwd_gen:N=-1': -1, 'frame_bwd_gen:nrows=-1': -1, 'frame_bwd_gen:W=-1': -1,
    'frame_bwd_gen:Nattr=-1': -1, 'frame_bwd_gen:K=0': -1, 'frame_bwd_gen:K=-1': -1, 'frame_bwd_gen:C=0': -1, 'frame_bwd_gen:C=5': -1,
    'frame_bwd_gen:form=-1': -1, 'frame_bwd_gen:form=3': -1, 'frame_bwd_gen:form=2,C=0,short': -2, 'frame_bwd_gen:form=2,K=cap+1': -3,
    'frame_bwd_gen:form=2,K=129,short': -2, 'frame_bwd_gen:kind=0': -1, 'frame_bwd_gen:kind=3': -1, 'frame_bwd_gen:kind=1,act,dsd': -1,
    'frame_bwd_gen:kind=1,act,dsd,short': -1, 'frame_bwd_gen:kind=1,short': -2, 'frame_bwd_gen:kind=1,form=2,short': -2,
    'frame_bwd_gen:kind=1,form=2,K=129,short': -2, 'frame_bwd_gen:K=cap+1': -3, 'frame_bwd_gen:K=cap+1,short': -3,
    'frame_bwd_gen:K=cap,short': -2, 'frame_bwd_gen:records=NULL,short': -1, 'frame_bwd_gen:rays=NULL,short': -1,
    'frame_bwd_gen:attr=NULL,short': -1, 'frame_bwd_gen:idx=NULL,short': -1, 'frame_bwd_gen:cnt=NULL,short': -1,
    'frame_bwd_gen:weight=NULL,short': -1, 'frame_bwd_gen:act=NULL,short': -1, 'frame_bwd_gen:len=NULL,short': -1,
    'frame_bwd_gen:dsd=NULL,short': -1, 'frame_bwd_gen:rgb=NULL,short': -1, 'frame_bwd_gen:wsum=NULL,short': -1,
    'frame_bwd_gen:bg=NULL,short': -1, 'frame_bwd_gen:g=NULL,short': -1, 'frame_bwd_gen:g_hitlen=NULL,short': -2,
    'frame_bwd_gen:ws=NULL,short': -1, 'frame_bwd_gen:g_verts=NULL,short': -1, 'frame_bwd_gen:g_sigmas=NULL,short': -1,
    'frame_bwd_gen:g_attr=NULL,short': -2, 'frame_bwd_gen:records=NULL': -1, 'frame_bwd_gen:rays=NULL': -1,
    'frame_bwd_gen:attr=NULL': -1, 'frame_bwd_gen:idx=NULL': -1, 'frame_bwd_gen:cnt=NULL': -1, 'frame_bwd_gen:weight=NULL': -1,
    'frame_bwd_gen:len=NULL': -1, 'frame_bwd_gen:rgb=NULL': -1, 'frame_bwd_gen:wsum=NULL': -1, 'frame_bwd_gen:bg=NULL': -1,
    'frame_bwd_gen:g=NULL': -1, 'frame_bwd_gen:ws=NULL': -1, 'frame_bwd_gen:act,no dsd': -1, 'frame_bwd_gen:dsd,no act': -1,
    'frame_bwd_gen:act,no dsd,short': -1, 'frame_bwd_gen:g_verts,no g_sigmas': -1, 'frame_bwd_gen:g_sigmas,no g_verts': -1,
    'frame_bwd_gen:neither g_verts nor g_sigmas,short': -2, 'frame_bwd_gen:short': -2, 'frame_bwd_gen:P=2^26': -1,
    'frame_bwd_gen:P=2^26,short': -2, 'frame_bwd_gen:Nattr*C=2^30': -1, 'frame_bwd_gen:Nattr*C=2^30,C=1': -1,
    'frame_bwd_gen:Nattr*C=2^30,short': -2, 'frame_bwd_gen:form=2,Nattr*C=2^30,short': -2, 'frame_bwd_gen:P=0,no outputs': 0,
    'frame_bwd_gen:P=0,no pointers,short': 0, 'frame_bwd_gen:P=0,K=cap+1': -3, 'frame_bwd_gen:N=0,no outputs': 0,
    'frame_bwd_gen:N=0,no pointers,short': 0, 'frame_bwd_gen:N=0,K=cap+1': -3, 'frame_bwd_gen:B=0,N=0,no outputs': 0,
    'frame_bwd_gen:B=0,N=0,no pointers,short': 0, 'frame_bwd_gen:B=0,N=0,K=cap+1': -3, 'frame_bwd_gen:nrows=0,no outputs': 0,
    'frame_bwd_gen:nrows=0,no pointers,short': 0, 'frame_bwd_gen:nrows=0,K=cap+1': -3, 'frame_bwd_gen:W=0,no outputs': 0,
    'frame_bwd_gen:W=0,no pointers,short': 0, 'frame_bwd_gen:W=0,K=cap+1': -3, 'frame_bwd_ori:B=-1': -1, 'frame_bwd_ori:N=-1': -1,
    'frame_bwd_ori:nrows=-1': -1, 'frame_bwd_ori:W=-1': -1, 'frame_bwd_ori:Nattr=-1': -1, 'frame_bwd_ori:K=0': -1,
    'frame_bwd_ori:K=-1': -1, 'frame_bwd_ori:C=0': -1, 'frame_bwd_ori:C=5': -1, 'frame_bwd_ori:sigma_mode=-1': -1,
    'frame_bwd_ori:sigma_mode=0': -1, 'frame_bwd_ori:sigma_mode=3': -1, 'frame_bwd_ori:form=-1': -1, 'frame_bwd_ori:form=3': -1,
    'frame_bwd_ori:form=2,C=0,short': -2, 'frame_bwd_ori:form=2,K=cap+1': -3, 'frame_bwd_ori:form=2,K=129,short': -2,
    'frame_bwd_ori:K=cap+1': -3, 'frame_bwd_ori:K=cap+1,short': -3, 'frame_bwd_ori:K=cap,short': -2,
    'frame_bwd_ori:records=NULL,short': -1, 'frame_bwd_ori:scales=NULL,short': -1, 'frame_bwd_ori:quats=NULL,short': -1,
    'frame_bwd_ori:rays=NULL,short': -1, 'frame_bwd_ori:attr=NULL,short': -1, 'frame_bwd_ori:idx=NULL,short': -1,
    'frame_bwd_ori:cnt=NULL,short': -1, 'frame_bwd_ori:weight=NULL,short': -1, 'frame_bwd_ori:act=NULL,short': -1,
    'frame_bwd_ori:len=NULL,short': -1, 'frame_bwd_ori:dsd=NULL,short': -1, 'frame_bwd_ori:rgb=NULL,short': -1,
    'frame_bwd_ori:wsum=NULL,short': -1, 'frame_bwd_ori:bg=NULL,short': -1, 'frame_bwd_ori:g=NULL,short': -1,
    'frame_bwd_ori:g_hitlen=NULL,short': -2, 'frame_bwd_ori:ws=NULL,short': -1, 'frame_bwd_ori:g_verts=NULL,short': -1,
    'frame_bwd_ori:g_sigmas=NULL,short': -1, 'frame_bwd_ori:g_quats=NULL,short': -1, 'frame_bwd_ori:g_attr=NULL,short': -2,
    'frame_bwd_ori:records=NULL': -1, 'frame_bwd_ori:scales=NULL': -1, 'frame_bwd_ori:quats=NULL': -1, 'frame_bwd_ori:rays=NULL': -1,
    'frame_bwd_ori:attr=NULL': -1, 'frame_bwd_ori:idx=NULL': -1, 'frame_bwd_ori:cnt=NULL': -1, 'frame_bwd_ori:weight=NULL': -1,
    'frame_bwd_ori:len=NULL': -1, 'frame_bwd_ori:rgb=NULL': -1, 'frame_bwd_ori:wsum=NULL': -1, 'frame_bwd_ori:bg=NULL': -1,
    'frame_bwd_ori:g=NULL': -1, 'frame_bwd_ori:ws=NULL': -1, 'frame_bwd_ori:act,no dsd': -1, 'frame_bwd_ori:dsd,no act': -1,
    'frame_bwd_ori:act,no dsd,short': -1, 'frame_bwd_ori:g_verts,no g_sigmas': -1, 'frame_bwd_ori:g_sigmas,no g_verts': -1,
    'frame_bwd_ori:neither g_verts nor g_sigmas,short': -1, 'frame_bwd_ori:g_scales,no g_quats': -1,
    'frame_bwd_ori:g_quats,no g_scales': -1, 'frame_bwd_ori:quats off 16 bytes': -1, 'frame_bwd_ori:g_quats off 16 bytes': -1,
    'frame_bwd_ori:quats off 16 bytes,short': -1, 'frame_bwd_ori:quats off 16 bytes,no gradients,short': -2,
    'frame_bwd_ori:no scales,no gradients,short': -2, 'frame_bwd_ori:quats off 16 bytes,P=0': 0, 'frame_bwd_ori:short': -2,
    'frame_bwd_ori:P=2^26': -1, 'frame_bwd_ori:P=2^26,short': -2, 'frame_bwd_ori:Nattr*C=2^30': -1, 'frame_bwd_ori:Nattr*C=2^30,C=1': -1,
    'frame_bwd_ori:Nattr*C=2^30,short': -2, 'frame_bwd_ori:form=2,Nattr*C=2^30,short': -2, 'frame_bwd_ori:P=0,no outputs': 0,
    'frame_bwd_ori:P=0,no pointers,short': 0, 'frame_bwd_ori:P=0,K=cap+1': -3, 'frame_bwd_ori:N=0,no outputs': 0,
    'frame_bwd_ori:N=0,no pointers,short': 0, 'frame_bwd_ori:N=0,K=cap+1': -3, 'frame_bwd_ori:B=0,N=0,no outputs': 0,
    'frame_bwd_ori:B=0,N=0,no pointers,short': 0, 'frame_bwd_ori:B=0,N=0,K=cap+1': -3, 'frame_bwd_ori:nrows=0,no outputs': 0,
    'frame_bwd_ori:nrows=0,no pointers,short': 0, 'frame_bwd_ori:nrows=0,K=cap+1': -3, 'frame_bwd_ori:W=0,no outputs': 0,
    'frame_bwd_ori:W=0,no pointers,short': 0, 'frame_bwd_ori:W=0,K=cap+1': -3,
}


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def run(lib, entry, over):
    call = base(entry)
    call.update(over)
    return getattr(lib, entry)(*call.values())


def test_the_table_covers_every_entry_and_is_unique():
    rows = cases()
    assert len({i for i, _, _ in rows}) == len(rows) == len(EXPECTED)
    assert {e for _, e, _ in rows} == set(ARGS) and len(ARGS) == 11
    assert set(EXPECTED.values()) == {0, -1, -2, -3}      # (nothing in the table reaches HIP: its codes are positive)


def test_every_entry_returns_the_recorded_code(lib):
    got = {i: run(lib, entry, over) for i, entry, over in cases()}
    wrong = {i: (got[i], EXPECTED.get(i)) for i in got if got[i] != EXPECTED.get(i)}
    assert not wrong, f"(returned, recorded): {wrong}"
