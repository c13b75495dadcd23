"""Mesh to training data (the reference's data/ directory): OBJ/MTL in, the .npz that `sin3dm_amd.train --data_path` reads out."""
