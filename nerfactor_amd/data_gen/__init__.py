"""data_gen — the drivers that turn raw data into what the training stages read (reference: data_gen/)."""
