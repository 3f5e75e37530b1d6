"""Regenerate tests/golden/reference_index.json, the fixture of tests/test_citations.py:

    python tests/golden/make_citation_index.py <path to a checkout of the reference>

For every reference file the project cites it records the number of lines, and for every marker
text of test_citations.KEY the numbers of the lines that contain it.  No reference text is stored:
the markers are the ones the test already names.
"""

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from test_citations import FILES, KEY  # noqa: E402


def main(ref: Path) -> None:
    index = {}
    for name, rel in FILES.items():
        lines = (ref / rel).read_text().splitlines()
        marks = sorted({text for _, n, _, text in KEY if n == name})
        index[name] = {"path": rel, "lines": len(lines),
                       "markers": {t: [i for i, ln in enumerate(lines, 1) if t in ln] for t in marks}}
    (HERE / "reference_index.json").write_text(json.dumps(index, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
