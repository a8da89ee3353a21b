from openvoice_amd.se_extractor import get_se, get_se_many, hash_numpy_array  # noqa: F401
