"""data_gen.dtu_mvs — DTU multi-view-stereo scans into the surface buffers of the MVS route (reference: data_gen/dtu_mvs/)."""
