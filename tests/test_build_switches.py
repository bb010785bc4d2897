"""The list of build variants of the kernels, in one place.

Every identifier that a preprocessor conditional of topfusion_amd/csrc tests must be on the
allow-list below, and the allow-list holds nothing that no conditional tests: a new build switch
is added here on purpose, with what it is for.  The A/B switches that were measured, decided and
folded into the code must not come back under their old names.
"""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "topfusion_amd" / "csrc"
MICRO = ROOT / "tools" / "micro"

# what a conditional may test, and why it is still a build variant
ALLOWED = {
    "__HIPCC__",                 # tf_mesh.h: shared by device code and the host-only PLY writer
    # a supported fallback: =0 is the memory-model form of the ICP hand-off
    "IP_XCD_STORE",
    # diagnostic instrumentation read by a tool under tools/; never the product
    "TF_ICP_TIMING",             # per-phase ICP timestamps (make timing, tools/icp_timing.py)
    "TF_SV_STATS",               # tools/micro/svd_lanes.hip: rotation / fallback / batched-test counts
    "TF_SV_TIMING",              # tools/micro/svd_lanes.hip: cycles per level phase
    "TF_RAY_STATS",              # raycast step counts
    "TF_PAIR_TIMELINE",          # the raycast pair's per-workgroup timeline
    "TF_PTL_LOOKAHEAD",          # ... recorded only by launches that carry later frames' preprocessing
    "TF_INTEG_TIMELINE",         # the integration pass's per-workgroup timeline
    "TF_C3X",                    # integration with parts of its traffic removed (results wrong)
    "TF_DIAG_NOP_AFTER_ICP",     # an empty launch after ICP (dispatch-gap diagnosis)
    # tuning constants, not A/Bs
    "ED_WIDE",
    "TF_INTEG_STREAM_BLOCKS",
    "TF_INTEG_RGB_WAVES",
    "TF_INTEG_PASS_WAVES",
}

# decided A/B switches, folded into the code: the kept form is the only form
RETIRED = [
    "IP_SVD_LANES", "IP_TAIL_ROWS", "IP_DET_WINDOW", "IP_OK_BITWISE", "IP_PCOPY", "IP_SLEEP",
    "TF_PROJ_DIV", "TF_RCP_BRANCH", "TF_SOLVE_LDL", "TF_RODRIGUES_SINC",
    "SV_WQ_BPERM", "SV_CS_W0", "SV_CS_LATE", "SV_CH_MASK", "SV_BCAST2", "SV_XOR_PARTNER", "SV_ONESHOT",
    "TF_INTEG_DIV", "TF_INTEG_LANEMAP", "TF_INTEG_NT_STORES",
    "TF_NORMAL_PHASES", "TF_ICP_EV_SYSFENCE",
]

COND = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$", re.M)
IDENT = re.compile(r"[A-Za-z_]\w*")
SOURCE_SUFFIXES = {".h", ".hip", ".cpp", ".c", ".py", ".sh", ".md", ".txt"}


def conditional_identifiers():
    found = {}
    files = [p for p in sorted(CSRC.iterdir()) if p.suffix in (".h", ".hip", ".cpp")]
    assert files, CSRC
    for p in files:
        text = p.read_text()
        for m in COND.finditer(text):
            expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            for name in IDENT.findall(expr):
                if name != "defined":
                    found.setdefault(name, p.name)
    return found


def test_conditionals_test_only_the_allowed_names():
    found = conditional_identifiers()
    extra = {n: f for n, f in found.items() if n not in ALLOWED}
    assert not extra, f"build switches not on the allow-list (name: first file): {extra}"
    unused = sorted(ALLOWED - set(found))
    assert not unused, f"allow-list entries that no conditional tests: {unused}"


def test_retired_switches_stay_retired():
    pat = re.compile(r"\b(" + "|".join(RETIRED) + r")\b")
    hits = []
    for d in (CSRC, MICRO):
        for p in sorted(d.rglob("*")):
            if not p.is_file() or not (p.suffix in SOURCE_SUFFIXES or p.name == "Makefile"):
                continue
            for k, line in enumerate(p.read_text(errors="replace").splitlines(), 1):
                if pat.search(line):
                    hits.append(f"{p.relative_to(ROOT)}:{k}: {line.strip()[:100]}")
    assert not hits, "retired build switches named again:\n" + "\n".join(hits)
