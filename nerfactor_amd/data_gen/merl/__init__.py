"""data_gen.merl — MERL `.binary` tables into the data directory of the BRDF prior (reference: data_gen/merl/)."""
