"""Data the package ships (the SRN test cameras) and the loaders of what a user brings (pointclouds.py)."""
