"""tests/cpp/refstub restates DECLARATIONS of the reference (so that the reference-side binding can be compile-checked in
an image without Eigen / iDynTree / BLF).  Every member the stand-ins declare must be one the reference's own header
declares: same return type, same parameter list, same cv-qualifier.  The reference's headers are not part of this
repository, so the check reads tests/golden/refstub_declarations.json: per header, the SHA-256 of every stand-in
signature that was found, whitespace removed, in the reference header's text.  A stand-in signature that drifts has no
digest there.  Regenerate the fixture from the reference's utils/include directory with

    python tests/test_refstub_signatures.py <reference>/src/flight-controller/utils/include

And the code block of INTEGRATION.md section 2 must be tests/cpp/integration_snippet.cpp, verbatim."""
import hashlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "cpp", "refstub")
FIXTURE = os.path.join(ROOT, "tests", "golden", "refstub_declarations.json")
HEADERS = ("QPInput.h", "Robot.h", "TrajectoryManager.h")


def _norm(text):
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def _public_member_declarations(stub_text):
    """signatures of the stand-in's public members that mirror the reference (everything before the first test* loader)"""
    body = stub_text[stub_text.index("public:") + len("public:"):]
    cut = [body.find(m) for m in ("// ---- test", "private:") if body.find(m) >= 0]
    body = _norm(body[:min(cut)])
    # <return type> name(<params>) [const]   followed by an inline body
    pat = re.compile(r"((?:const )?[\w:<>, ]+?[&\*]?) (\w+)\(([^()]*)\)( const)? \{")
    out = []
    for m in pat.finditer(body):
        ret, name, params, cv = m.group(1).strip(), m.group(2), m.group(3).strip(), (m.group(4) or "").strip()
        if name in ("if", "for", "while", "switch"):
            continue
        out.append((ret, name, params, cv))
    return out


def _stub_signatures(header):
    """the stand-in's public member declarations as `ret name(params) [const];`, all whitespace removed"""
    decls = _public_member_declarations(open(os.path.join(STUB, header)).read())
    return [f"{ret} {name}({params}){' ' + cv if cv else ''};".replace(" ", "") for ret, name, params, cv in decls]


def _digest(sig):
    return hashlib.sha256(sig.encode()).hexdigest()


@pytest.mark.parametrize("header, expect_at_least", [("QPInput.h", 18), ("Robot.h", 19), ("TrajectoryManager.h", 5)])
def test_stub_declarations_are_the_references(header, expect_at_least):
    verified = set(json.load(open(FIXTURE))[header])
    sigs = _stub_signatures(header)
    assert len(sigs) >= expect_at_least, sigs
    missing = [sig for sig in sigs if _digest(sig) not in verified]
    assert not missing, f"{header}: not declared like this in the reference: {missing}"


def test_integration_md_shows_the_compiled_snippet_verbatim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    snippet = open(os.path.join(ROOT, "tests", "cpp", "integration_snippet.cpp")).read().strip()
    blocks = re.findall(r"```cpp\n(.*?)```", doc, flags=re.S)
    assert any(b.strip() == snippet for b in blocks), "INTEGRATION.md section 2 must carry tests/cpp/integration_snippet.cpp verbatim"


def record_reference_declarations(ref_utils):
    """writes FIXTURE from the reference's utils/include directory; refuses if a stand-in signature is not declared there"""
    out = {}
    for header in HEADERS:
        # the reference breaks lines inside declarations: compare with all whitespace removed
        ref = _norm(open(os.path.join(ref_utils, header)).read()).replace(" ", "")
        sigs = _stub_signatures(header)
        missing = [sig for sig in sigs if sig not in ref]
        if missing:
            raise SystemExit(f"{header}: not declared like this in the reference: {missing}")
        out[header] = sorted({_digest(sig) for sig in sigs})
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    record_reference_declarations(sys.argv[1])
