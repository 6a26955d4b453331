"""Writes tests/golden/text_query.npz: the reference's 20 ScanNet class names and their (20, 768) fp32 SigLIP2 text embeddings (data of
the reference: pointcept/datasets/preprocessing/scannet/meta_data/scannet20_labels.txt and scannet20_text_embeddings_siglip2.pt), and
a seeded feature set built from them (tests/text_query_cases.fixture_features: 600 rows, each a class embedding plus noise, stored
fp16, with its class id).  Run on the CPU:

    python tests/golden/make_golden_text_query.py <path of the reference tree>

Only data is written; no reference source."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import text_query_cases as tc  # noqa: E402

META = os.path.join("pointcept", "datasets", "preprocessing", "scannet", "meta_data")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    meta = os.path.join(sys.argv[1], META)
    with open(os.path.join(meta, "scannet20_labels.txt")) as f:
        names = [line.strip() for line in f if line.strip()]
    emb = torch.load(os.path.join(meta, "scannet20_text_embeddings_siglip2.pt"), map_location="cpu", weights_only=True).float().numpy()
    assert emb.shape == (len(names), 768) and len(names) == 20, (emb.shape, len(names))
    features, cls = tc.fixture_features(emb)
    np.savez_compressed(tc.GOLDEN, class_names=np.array(names), embeddings=emb.astype(np.float32), features=features, class_id=cls)
    print(f"wrote {tc.GOLDEN}: {os.path.getsize(tc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
